"""CPU: the frame kernels themselves (sqz_amd/csrc/frame.hip: checksums, index construction, index validation),
compiled by g++ against tests/emu/hip/hip_runtime.h and run lane by lane on the CPU wave emulator, held against
zlib.crc32 and the independent frame writer (tests/frame_writer.py).  This pins the kernels' LOGIC without a GPU;
the -m gpu tests pin the gfx950 build."""
import ctypes as C
import errno
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import frame_writer as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
LENGTHS = [0, 1, 3, 63, 64, 65, 255, 4095, 4096, 4097, 70001]


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU, "libsqz_emu_frame.so")
    deps = [os.path.join(EMU, f) for f in ("emu_runtime.cpp", "emu_frame.cpp", "hip/hip_runtime.h")] + \
           [os.path.join(CSRC, f) for f in ("frame.hip", "sqz_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-I" + EMU,
                               "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                               "-Wno-attributes", os.path.join(EMU, "emu_runtime.cpp"),
                               os.path.join(EMU, "emu_frame.cpp"), "-o", out])
    return C.CDLL(out)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def aligned_copy(data: bytes):
    """the bytes in a buffer that starts on a 16-byte boundary (what the device entry points ask of a frame)"""
    raw = np.zeros(len(data) + 64 + 16, np.uint8)
    buf = raw[(-raw.ctypes.data) % 16:]
    buf[:len(data)] = np.frombuffer(data, np.uint8)
    return buf


def crc_ranges(E, buf, offsets, hint=0):
    off = np.asarray(offsets, np.uint64)
    crc = np.full(len(off) - 1, 0xDEADBEEF, np.uint32)
    E.emu_crc32_blocks(_p(buf), _p(off), len(off) - 1, _p(crc), C.c_uint64(hint))
    return crc.tolist()


def test_crc_equals_zlib_at_every_length_and_alignment(emu):
    raw = np.random.default_rng(5).integers(0, 256, 70001 + 64 + 16, dtype=np.uint8)
    buf = raw[(-raw.ctypes.data) % 16:]                      # buf[0] on a 16-byte boundary: `start` IS the misalignment
    assert buf.ctypes.data % 16 == 0
    for n in LENGTHS:
        for start in range(18):
            want = zlib.crc32(buf[start:start + n].tobytes())
            # the launch's three shapes: size unknown (the most workgroups, most of them leave at once), size
            # known (one workgroup per 64 KB), and a batch big enough for one workgroup per range
            assert crc_ranges(emu, buf, [start, start + n]) == [want], (n, start)
            if start in (0, 1, 15, 17):
                assert crc_ranges(emu, buf, [start, start + n], hint=n) == [want], (n, start)


def test_crc_of_a_ragged_batch(emu):
    rng = np.random.default_rng(6)
    buf = rng.integers(0, 256, 300000, dtype=np.uint8)
    cuts = sorted(set([0, 5, 5, 4100, 30000, 30001, 98304 + 7, 300000] + rng.integers(0, 300000, 40).tolist()))
    cuts = [0, 5, 5] + cuts[2:]                              # an empty range inside the batch
    want = [zlib.crc32(buf[a:b].tobytes()) for a, b in zip(cuts, cuts[1:])]
    assert crc_ranges(emu, buf, cuts) == want
    assert crc_ranges(emu, buf, cuts, hint=300000) == want
    big = [0] * 5000                                         # more ranges than the launch has workgroups to share
    assert crc_ranges(emu, buf, big + [300000])[-1] == zlib.crc32(buf.tobytes())
    assert crc_ranges(emu, buf, [7, 3]) == [0]               # an inverted pair counts as empty


def index_inputs(frame):
    f = W.fields(frame)
    n = f["n_blocks"]
    idx = np.frombuffer(frame[32:32 + 8 * n], np.uint32).reshape(n, 2) if n else np.zeros((0, 2), np.uint32)
    return f, n, (idx[:, 0].astype(np.uint64) * 8), idx[:, 1].copy()


def run_index(E, frame, capacity=None, err=None):
    f, n, sizes, crcs = index_inputs(frame)
    capacity = f["frame_bytes"] if capacity is None else capacity
    out = np.full(f["frame_bytes"] + 64, 0xA5, np.uint8)
    out = out[(-out.ctypes.data) % 16:]
    sizes_a = np.concatenate([sizes, np.zeros(1, np.uint64)])
    crcs_a = np.concatenate([crcs, np.zeros(1, np.uint32)])
    err_a = np.zeros(n + 1, np.int32) if err is None else np.asarray(err, np.int32)
    copy_bytes, dense_off = np.full(n + 1, 77, np.uint64), np.full(n + 2, 77, np.uint64)
    fb, st = np.zeros(1, np.uint64), np.full(1, -1, np.int32)
    E.emu_frame_index(_p(sizes_a), _p(err_a), _p(crcs_a), n, C.c_uint64(f["content_bytes"]), f["win_bits"],
                      f["block_bytes"].bit_length() - 1, _p(out), C.c_uint64(capacity), _p(copy_bytes),
                      _p(dense_off), _p(fb), _p(st))
    return f, n, sizes, out, copy_bytes[:n], dense_off[:n + 1], int(fb[0]), int(st[0])


@pytest.mark.parametrize("name", W.CASE_IDS)
def test_index_kernel_writes_the_writers_header_and_index(emu, name):
    frame = W.case_frame(name)
    f, n, sizes, out, copy_bytes, dense_off, fb, st = run_index(emu, frame)
    assert st == 0 and fb == len(frame)
    assert out[:f["payload_off"]].tobytes() == frame[:f["payload_off"]]
    assert (out[f["payload_off"]:f["frame_bytes"]] == 0xA5).all()       # the payload is the compaction's
    assert copy_bytes.tolist() == sizes.tolist()
    assert dense_off.tolist() == (f["payload_off"] + np.concatenate([[0], np.cumsum(sizes)])).astype(np.uint64).tolist()


def test_index_kernel_refuses_without_writing(emu):
    frame = W.case_frame("laozi_w15_b12")
    for kw, want in (({"capacity": len(frame) - 1}, errno.E2BIG), ({"capacity": 0}, errno.E2BIG),
                     ({"err": [0, 0, errno.EINVAL] + [0] * 30}, errno.EINVAL)):
        f, n, sizes, out, copy_bytes, dense_off, fb, st = run_index(emu, frame, **kw)
        assert st == want and fb == len(frame)                      # the size needed is still reported
        assert (out == 0xA5).all() and not copy_bytes.any() and not dense_off.any()


def run_open(E, frame, n, content, first=0, n_sel=None, avail=None):
    n_sel = n - first if n_sel is None else n_sel
    buf = aligned_copy(frame)
    in_off, out_off = np.full(n_sel + 1, 99, np.uint64), np.full(n_sel + 1, 99, np.uint64)
    st = np.full(1, -1, np.int32)
    rc = E.emu_frame_open(_p(buf), C.c_uint64(len(frame) if avail is None else avail), n, C.c_uint64(content), first,
                          n_sel, _p(in_off), _p(out_off), _p(st))
    return rc, int(st[0]), in_off.tolist(), out_off.tolist()


@pytest.mark.parametrize("name", W.CASE_IDS)
def test_open_kernel_builds_the_offsets(emu, name):
    frame = W.case_frame(name)
    f, n, sizes, _ = index_inputs(frame)
    starts = (f["payload_off"] + np.concatenate([[0], np.cumsum(sizes)])).astype(np.uint64).tolist()
    bb, content = f["block_bytes"], f["content_bytes"]
    rc, st, in_off, out_off = run_open(emu, frame, n, content)
    assert (rc, st) == (0, 0)
    assert in_off == starts and out_off == [min(k * bb, content) for k in range(n + 1)]
    if n >= 3:                                               # a block range, as sqz_frame_read asks for
        for first, n_sel in ((1, 1), (n - 1, 1), (1, n - 1), (0, 2)):
            rc, st, in_off, out_off = run_open(emu, frame, n, content, first, n_sel)
            assert (rc, st) == (0, 0)
            assert in_off == starts[first:first + n_sel + 1]
            assert out_off == [min((first + k) * bb, content) - first * bb for k in range(n_sel + 1)]


def test_open_kernel_refusals(emu):
    frame = W.case_frame("laozi_w15_b12")
    good = W.fields(frame)
    for name, bad, head_errno, full_errno in W.refusals(frame):
        # what a caller passes: the header's own figures where the header alone parses, the good frame's otherwise
        src = W.fields(bad) if head_errno == 0 else good
        rc, st, in_off, out_off = run_open(emu, bad, good["n_blocks"], src["content_bytes"])
        assert rc == 0 and st == (full_errno if head_errno == 0 else errno.EINVAL), name
        assert not any(in_off) and not any(out_off), name    # zero-length input and output for every block
    n, content = good["n_blocks"], good["content_bytes"]
    rc, st, in_off, out_off = run_open(emu, frame, n, content, avail=len(frame) - 8)
    assert (rc, st) == (0, errno.E2BIG) and not any(in_off) and not any(out_off)
    rc, st, in_off, out_off = run_open(emu, frame, n, content, first=2, n_sel=n - 1)     # a range beyond the frame
    assert (rc, st) == (0, errno.EINVAL) and not any(in_off)
    # stream sizes that add up to more than any buffer holds: refused by arithmetic, no wrap
    b = bytearray(frame)
    for k in range(n):
        struct.pack_into("<I", b, 32 + 8 * k, 0xFFFFFFFF)
    rc, st, in_off, out_off = run_open(emu, W.reseal(b), n, content)
    assert (rc, st) == (0, errno.E2BIG) and not any(in_off)


def test_verify_kernel(emu):
    frame = W.case_frame("laozi_w15_b12")
    f, n, sizes, crcs = index_inputs(frame)
    buf = aligned_copy(frame)
    got = crcs.copy()
    got[3] ^= 1                                              # block 3 decoded to other bytes
    err = np.zeros(n, np.int32)
    err[5] = errno.E2BIG                                     # the decoder's own verdict stays
    got[5] ^= 1
    st = np.zeros(1, np.int32)
    emu.emu_frame_verify(_p(buf), 0, n, _p(got), _p(st), _p(err))
    want = [0] * n
    want[3], want[5] = errno.EILSEQ, errno.E2BIG
    assert err.tolist() == want
    err2 = np.zeros(2, np.int32)                             # a block range: entries 4 and 5 of the index
    emu.emu_frame_verify(_p(buf), 4, 2, _p(got[4:6].copy()), _p(st), _p(err2))
    assert err2.tolist() == [0, errno.EILSEQ]
    st[0] = errno.EILSEQ                                     # a refused frame: every block says so
    emu.emu_frame_verify(_p(buf), 0, n, _p(crcs), _p(st), _p(err))
    assert err.tolist() == [errno.EILSEQ] * n
