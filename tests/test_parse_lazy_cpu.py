"""CPU, no device: the parse argument at the edges of the interface -- the values the _parse calls refuse (before
anything is launched or written), the names the Python layer refuses, the tool's --lazy option, and the model
(tests/lazy_model.py) against the oracle where the two must agree."""
import ctypes as C
import errno

import numpy as np
import pytest

import lazy_model as LM
import oracle_lib as O


@pytest.fixture(scope="module")
def lib():
    from sqz_amd import build, _native
    build.build_native()
    return _native.lib()


def _calls(lib, parse, finder=1):
    """every _parse call with arguments that would pass if `parse` did: host arrays where a host call looks at
    them, a non-null word where a device pointer is only checked for being one"""
    buf = np.zeros(4096, np.uint8)
    off = np.array([0, 64], np.uint64)
    out_off = np.array([0, 1024], np.uint64)
    out_bytes = np.full(1, 0xAAAAAAAA, np.uint64)
    err = np.full(1, 0x55555555, np.int32)
    nbytes = C.c_uint64(0xAAAAAAAA)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dev = C.c_void_p(4096)                                       # never dereferenced by a refused call
    res = {
        "sqz_encode_blocks_parse": lib.sqz_encode_blocks_parse(p(buf), p(off), 1, 1 << 15, parse, p(buf), p(out_off),
                                                               p(out_bytes), p(err)),
        "sqz_hip_encode_blocks_parse": lib.sqz_hip_encode_blocks_parse(dev, dev, 1, 1 << 15, parse, dev, dev, dev, dev,
                                                                       dev, 1 << 20, None),
        "sqz_hip_lz77_blocks_parse": lib.sqz_hip_lz77_blocks_parse(dev, dev, 1, 1 << 15, dev, dev, finder, parse, dev,
                                                                   1 << 20, None),
        "sqz_frame_compress_parse": lib.sqz_frame_compress_parse(p(buf), 64, 15, 12, 0, parse, p(buf), 4096,
                                                                 C.byref(nbytes)),
        "sqz_hip_frame_encode_parse": lib.sqz_hip_frame_encode_parse(dev, 64, 15, 12, 0, parse, dev, 4096, dev, dev,
                                                                     dev, dev, 1 << 20, None),
    }
    untouched = int(out_bytes[0]) == 0xAAAAAAAA and int(err[0]) == 0x55555555 and nbytes.value == 0xAAAAAAAA and \
        not buf.any()
    return res, untouched


@pytest.mark.parametrize("parse", [2, 0x80, 0xFFFFFFFF])
def test_an_unknown_parse_is_refused_by_every_call(lib, parse):
    res, untouched = _calls(lib, parse)
    assert res == {name: errno.EINVAL for name in res}
    assert untouched


def test_the_scan_finder_has_no_lazy_parse(lib):
    dev = C.c_void_p(4096)
    assert lib.sqz_hip_lz77_blocks_parse(dev, dev, 1, 1 << 15, dev, dev, 0, 1, dev, 1 << 20, None) == errno.EINVAL
    assert lib.sqz_hip_lz77_blocks_parse(dev, dev, 1, 1 << 15, dev, dev, 0, 1, None, 0, None) == errno.EINVAL
    assert lib.sqz_hip_lz77_blocks_parse(dev, dev, 1, 1 << 15, dev, dev, 2, 1, dev, 1 << 20, None) == errno.EINVAL


def test_the_constants_of_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sqz", "sqz.h")).read()
    assert re.search(r"#define\s+SQZ_PARSE_GREEDY\s+0u\b", text) and re.search(r"#define\s+SQZ_PARSE_LAZY\s+1u\b", text)
    from sqz_amd import codec
    assert (codec.PARSE_GREEDY, codec.PARSE_LAZY) == (0, 1)
    assert codec.parse_code("greedy") == 0 and codec.parse_code("lazy") == 1


@pytest.mark.parametrize("bad", ["x", "", "LAZY", None, 1])
def test_python_refuses_other_names(lib, bad):
    from sqz_amd import batch, codec, frame
    with pytest.raises(ValueError):
        codec.parse_code(bad)
    with pytest.raises(ValueError):
        frame.compress_frame(b"abc" * 100, 15, 12, parse=bad)
    with pytest.raises(ValueError):
        batch.encode_blocks_host([b"abc" * 100], 1 << 15, parse=bad)
    with pytest.raises(ValueError):
        frame.FrameEncoder(4096, 15, 12, device="cpu", parse=bad)
    with pytest.raises(ValueError):                              # (nothing of the object is needed to refuse)
        batch.Encoder.encode(None, None, None, 1 << 15, parse=bad)
    with pytest.raises(ValueError):
        batch.Encoder.tokens(None, None, None, 1 << 15, parse=bad)
    with pytest.raises(ValueError):
        batch.Encoder.tokens(None, None, None, 1 << 15, finder="scan", parse="lazy")


def test_the_tool_takes_lazy(lib, tmp_path, monkeypatch):
    from sqz_amd import frame
    seen = []

    def fake(data, win_bits=15, block_bits=18, store=False, parse="greedy"):
        seen.append((bytes(data), win_bits, block_bits, store, parse))
        return b"frame"

    monkeypatch.setattr(frame, "compress_frame", fake)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.write_bytes(b"content")
    assert frame.main(["c", str(src), str(dst), "--lazy"]) == 0
    assert frame.main(["c", str(src), str(dst), "--win-bits", "12", "--block-bits", "14", "--store", "--lazy"]) == 0
    assert frame.main(["c", str(src), str(dst)]) == 0
    assert seen == [(b"content", 15, 18, False, "lazy"), (b"content", 12, 14, True, "lazy"),
                    (b"content", 15, 18, False, "greedy")]
    assert dst.read_bytes() == b"frame"
    with pytest.raises(SystemExit):
        frame.main(["d", str(src), str(dst), "--lazy"])           # an option of the compress command only


@pytest.mark.parametrize("name,cut,window", [("laozi.txt", 3000, 1 << 10), ("x64.elf", 2500, 1 << 12)])
def test_the_model(name, cut, window):
    """its greedy branch is the oracle's token sequence; its lazy stream decodes to the input -- through the
    restatement's decoder and, where it is built, the compiled reference's"""
    data = O.corpus(name)[:cut]
    tab = LM.table(data, window)
    greedy, none = LM.parse(data, window, False, tab)
    assert none == [] and (greedy == O.tokens(data, window)).all()
    assert LM.stream(greedy) == O.encode(data, 0, header=False, window=window)
    lazy, gave = LM.parse(data, window, True, tab)
    assert len(gave) > 0
    comp = LM.stream(lazy)
    e, back, _ = O.decode(comp, header=False, nbytes=len(data))
    assert e == 0 and back == data
    if O.REF is not None:
        out = C.create_string_buffer(len(data))
        n, wb = C.c_uint64(len(data)), C.c_int(0)
        assert O.REF.sqz_ref_decompress(comp, len(comp), 0, out, len(data), C.byref(n), C.byref(wb)) == 0
        assert out.raw[:len(data)] == data
