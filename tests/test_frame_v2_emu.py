"""CPU: what SQZF version 2 (stored blocks) adds to the kernels -- the ragged range copy, the version-2 flavours of the
index and open kernels (sqz_amd/csrc/frame.hip), the decode kernels' skip mask (decode.hip) -- compiled by g++ against
tests/emu/hip/hip_runtime.h and run lane by lane on the CPU wave emulator, held against the independent version-2
writer (tests/frame_writer_v2.py).  This pins the kernels' LOGIC without a GPU; the -m gpu tests pin the gfx950
build."""
import ctypes as C
import errno
import os
import struct
import subprocess

import numpy as np
import pytest

import frame_writer as W
import frame_writer_v2 as W2
from test_frame_emu import LENGTHS, aligned_copy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
GUARD = 24


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU, "libsqz_emu_frame_v2.so")
    deps = [os.path.join(EMU, f) for f in ("emu_runtime.cpp", "emu_frame_v2.cpp", "hip/hip_runtime.h")] + \
           [os.path.join(CSRC, f) for f in ("frame.hip", "decode.hip", "sqz_tree.h", "sqz_device.h", "sqz_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-I" + EMU,
                               "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                               "-Wno-attributes", os.path.join(EMU, "emu_runtime.cpp"),
                               os.path.join(EMU, "emu_frame_v2.cpp"), "-o", out])
    return C.CDLL(out)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def aligned(n, fill):
    raw = np.full(n + 16, fill, np.uint8)
    return raw[(-raw.ctypes.data) % 16:][:n]


# ---------------------------------------------------------------------------------- the copy kernel
def run_copy(E, src, src_off, dst, dst_off, len_from_dst, mask, pad8, hint=0):
    so, do = np.asarray(src_off, np.uint64), np.asarray(dst_off, np.uint64)
    n = (len(do) if len_from_dst else len(so)) - 1
    m = None if mask is None else np.asarray(mask, np.uint32)
    E.emu_range_copy(_p(src), _p(so), _p(dst), _p(do), int(len_from_dst), _p(m), n, int(pad8), C.c_uint64(hint))


def test_copy_at_every_length_and_alignment(emu):
    most = max(LENGTHS)
    src = aligned(most + 64, 0)
    src[:] = np.random.default_rng(21).integers(0, 256, len(src), dtype=np.uint8)
    assert src.ctypes.data % 16 == 0
    for n in LENGTHS:
        # every pair of misalignments at every length: head, rows and tail all take part, and the longest length
        # runs several workgroups and the grid-stride loop more than once per lane
        for s, d in [(s, d) for s in range(18) for d in range(18)]:
            # the launch's shapes: size known (one workgroup per 32 KB), and, for a few pairs, size unknown (the most
            # workgroups, most of them with nothing to do)
            for pad8, hint in ((False, n), (True, n)) + (((True, 0),) if (s, d) in ((0, 0), (1, 8), (17, 3)) else ()):
                dst = aligned(n + 64 + 2 * GUARD, 0xA5)
                at = GUARD + d
                # the source's length from the source side (encode) and from the destination side (decode)
                run_copy(emu, src, [s, s + n], dst, [at, at + n], not pad8, None, pad8, hint)
                end = at + (W2.pad8(n) if pad8 else n)
                assert dst[at:at + n].tobytes() == src[s:s + n].tobytes(), (n, s, d, pad8)
                assert not dst[at + n:end].any(), (n, s, d)                                  # the padding: zeros
                assert (dst[:at] == 0xA5).all() and (dst[end:] == 0xA5).all(), (n, s, d, pad8)   # the guards


def test_copy_of_a_ragged_batch_with_a_predicate(emu):
    rng = np.random.default_rng(22)
    src = rng.integers(0, 256, 300000, dtype=np.uint8)
    cuts = sorted(set([0, 5, 4100, 30000, 30001, 98304 + 7, 300000] + rng.integers(0, 300000, 40).tolist()))
    cuts = [0, 5, 5] + cuts[2:]                              # an empty range inside the batch
    n = len(cuts) - 1
    mask = (rng.integers(0, 3, n) > 0).astype(np.uint32)     # a third of the ranges is left out
    mask[1] = 1                                              # the empty one is asked for
    assert 0 < int(mask.sum()) < n
    # encode shape: lengths from the source, each range lands padded to 8 at an 8-byte aligned place of its own
    lens = np.diff(np.asarray(cuts))
    dst_off = np.concatenate([[0], np.cumsum((lens + 7) // 8 * 8 + 8)]) + 8
    for hint in (0, 300000, 1):
        dst = aligned(int(dst_off[-1]) + 64, 0xA5)
        run_copy(emu, src, cuts, dst, dst_off[:n], False, mask, True, hint)
        want = np.full(len(dst), 0xA5, np.uint8)
        for b in range(n):
            if mask[b]:
                want[dst_off[b]:dst_off[b] + lens[b]] = src[cuts[b]:cuts[b + 1]]
                want[dst_off[b] + lens[b]:dst_off[b] + (lens[b] + 7) // 8 * 8] = 0
        assert (dst == want).all(), hint
    # decode shape: lengths from the destination, ranges back to back at any alignment, nothing padded
    src_off = (np.cumsum(np.concatenate([[0], (lens + 7) // 8 * 8]))[:n]).astype(np.uint64)
    packed = np.zeros(int(src_off[-1]) + 300000, np.uint8)
    for b in range(n):
        packed[int(src_off[b]):int(src_off[b]) + lens[b]] = src[cuts[b]:cuts[b + 1]]
    dst = aligned(300000 + 64, 0xA5)
    out_off = np.asarray(cuts) + 3
    run_copy(emu, packed, src_off, dst, out_off, True, mask, False, 4096)
    want = np.full(len(dst), 0xA5, np.uint8)
    for b in range(n):
        if mask[b]:
            want[out_off[b]:out_off[b + 1]] = src[cuts[b]:cuts[b + 1]]
    assert (dst == want).all()
    none = aligned(64, 0xA5)                                 # a mask that leaves everything out; n = 0
    run_copy(emu, src, [0, 40], none, [8, 48], False, [0], True)
    run_copy(emu, src, [0], none, [0], False, None, True)
    assert (none == 0xA5).all()


# ---------------------------------------------------------------------------------- the index kernel
def run_index(E, name, capacity=None, err=None):
    frame, data = W2.case_frame(name), W2.case_data(name)
    f, blk = W2.fields(frame), W2.blocks(frame)
    n = f["n_blocks"]
    sizes = np.asarray([len(s) for s in W2.case_streams(name)] + [0], np.uint64)
    crcs = np.asarray([b["content_crc"] for b in blk] + [0], np.uint32)
    capacity = len(frame) if capacity is None else capacity
    out = aligned(len(frame) + 64, 0xA5)
    err_a = np.zeros(n + 1, np.int32) if err is None else np.asarray(err, np.int32)
    copy_bytes, dense_off = np.full(n + 1, 77, np.uint64), np.full(n + 2, 77, np.uint64)
    stored = np.full(n + 1, 77, np.uint32)
    fb, st = np.zeros(1, np.uint64), np.full(1, -1, np.int32)
    E.emu_frame_index_v2(_p(sizes), _p(err_a), _p(crcs), n, C.c_uint64(len(data)), f["win_bits"],
                         f["block_bytes"].bit_length() - 1, _p(out), C.c_uint64(capacity), _p(copy_bytes),
                         _p(dense_off), _p(stored), _p(fb), _p(st))
    return frame, f, blk, sizes[:n], out, copy_bytes, dense_off, stored, int(fb[0]), int(st[0])


@pytest.mark.parametrize("name", W2.CASE_IDS)
def test_index_kernel_writes_the_writers_header_index_and_work_lists(emu, name):
    frame, f, blk, sizes, out, copy_bytes, dense_off, stored, fb, st = run_index(emu, name)
    n = f["n_blocks"]
    assert st == 0 and fb == len(frame)
    assert out[:f["payload_off"]].tobytes() == frame[:f["payload_off"]]
    assert (out[f["payload_off"]:] == 0xA5).all()                                # the payload is the copies'
    want_stored = [b["stored"] for b in blk]
    assert stored[:n].tolist() == want_stored and stored[n] == 77
    assert copy_bytes[:n].tolist() == [0 if s else int(v) for s, v in zip(want_stored, sizes)] and copy_bytes[n] == 77
    assert dense_off[:n + 1].tolist() == [b["payload_off"] for b in blk] + [len(frame)] and dense_off[n + 1] == 77
    # the two work lists are disjoint and together cover the payload: the compaction's and the copy's bytes
    moved = sum(int(c) for c in copy_bytes[:n]) + sum(W2.pad8(b["content_bytes"]) for b in blk if b["stored"])
    assert moved == f["payload_bytes"]


def test_index_kernel_refuses_without_writing(emu):
    name = "mandrill_bmp_w10_b18"
    size = len(W2.case_frame(name))
    for kw, want in (({"capacity": size - 1}, errno.E2BIG), ({"capacity": 0}, errno.E2BIG),
                     ({"err": [0, 0, errno.EINVAL, 0, 0]}, errno.EINVAL)):
        frame, f, blk, sizes, out, copy_bytes, dense_off, stored, fb, st = run_index(emu, name, **kw)
        n = f["n_blocks"]
        assert st == want and fb == size                             # the size needed is still reported
        assert (out == 0xA5).all() and not copy_bytes[:n].any() and not dense_off[:n + 1].any() and not stored[:n].any()
    # the capacity check uses the real size: a frame of noise fits the version-2 bound, not one byte less
    frame, f, blk, sizes, out, copy_bytes, dense_off, stored, fb, st = run_index(emu, "mandrill_png_w15_b14",
                                                                                 capacity=W2.case("mandrill_png_w15_b14")[8])
    assert st == 0 and all(stored[:f["n_blocks"]])


# ---------------------------------------------------------------------------------- the open kernel
def run_open(E, frame, n, content, first=0, n_sel=None, avail=None):
    n_sel = n - first if n_sel is None else n_sel
    buf = aligned_copy(frame)
    in_off, out_off = np.full(n_sel + 1, 99, np.uint64), np.full(n_sel + 1, 99, np.uint64)
    stored = np.full(n_sel + 1, 99, np.uint32)
    st = np.full(1, -1, np.int32)
    rc = E.emu_frame_open_v2(_p(buf), C.c_uint64(len(frame) if avail is None else avail), n, C.c_uint64(content), first,
                             n_sel, _p(in_off), _p(out_off), _p(stored), _p(st))
    assert stored[n_sel] == 99
    return rc, int(st[0]), in_off.tolist(), out_off.tolist(), stored[:n_sel].tolist()


@pytest.mark.parametrize("name", W2.CASE_IDS)
def test_open_kernel_builds_offsets_and_mask(emu, name):
    for frame in (W2.case_frame(name), W2.case_frame_v1(name)):              # this launcher takes both versions
        f, blk = W2.fields(frame), W2.blocks(frame)
        n, bb, content = f["n_blocks"], f["block_bytes"], f["content_bytes"]
        starts = [b["payload_off"] for b in blk] + [len(frame)]
        mask = [b["stored"] for b in blk]
        rc, st, in_off, out_off, stored = run_open(emu, frame, n, content)
        assert (rc, st) == (0, 0)
        assert in_off == starts and out_off == [min(k * bb, content) for k in range(n + 1)] and stored == mask
        if n >= 3:                                           # a block range, as sqz_frame_read asks for
            for first, n_sel in ((1, 1), (n - 1, 1), (1, n - 1), (0, 2)):
                rc, st, in_off, out_off, stored = run_open(emu, frame, n, content, first, n_sel)
                assert (rc, st) == (0, 0)
                assert in_off == starts[first:first + n_sel + 1] and stored == mask[first:first + n_sel]
                assert out_off == [min((first + k) * bb, content) - first * bb for k in range(n_sel + 1)]


@pytest.mark.parametrize("name", ["mandrill_bmp_w10_b18", "x64_w15_b12"])
def test_open_kernel_refusals(emu, name):
    frame = W2.case_frame(name)
    good = W2.fields(frame)
    n, content = good["n_blocks"], good["content_bytes"]
    both = [r for r in W.refusals(frame) if r[0] not in ("version_2", "flags_1")] + W2.refusals(frame)
    for what, bad, head_errno, full_errno in both:
        # what a caller passes: the header's own figures where the header alone parses, the good frame's otherwise
        src = W2.fields(bad) if head_errno == 0 else good
        rc, st, in_off, out_off, stored = run_open(emu, bad, n, src["content_bytes"])
        assert rc == 0 and st == (full_errno if head_errno == 0 else errno.EINVAL), what
        assert not any(in_off) and not any(out_off) and not any(stored), what   # zero-length ranges, nothing marked
    rc, st, in_off, out_off, stored = run_open(emu, frame, n, content, avail=len(frame) - 8)
    assert (rc, st) == (0, errno.E2BIG) and not any(in_off) and not any(out_off) and not any(stored)
    rc, st, in_off, out_off, stored = run_open(emu, frame, n, content, first=2, n_sel=n - 1)
    assert (rc, st) == (0, errno.EINVAL) and not any(in_off) and not any(stored)
    # sizes that add up to more than any buffer holds, stream entries and stored ones: refused by arithmetic
    for word, want in ((0x7FFFFFFF, errno.E2BIG), (0xFFFFFFFF, errno.EINVAL)):
        b = bytearray(frame)
        for k in range(n):
            struct.pack_into("<I", b, 32 + 8 * k, word)
        rc, st, in_off, out_off, stored = run_open(emu, W.reseal(b), n, content)
        assert (rc, st) == (0, want) and not any(in_off) and not any(stored)


def test_the_version_1_launcher_refuses_a_version_2_frame(emu):
    """the launcher without a mask keeps its meaning: version 1 only"""
    frame = W2.case_frame("mandrill_bmp_w10_b18")
    f = W2.fields(frame)
    n = f["n_blocks"]
    buf = aligned_copy(frame)
    in_off, out_off = np.full(n + 1, 99, np.uint64), np.full(n + 1, 99, np.uint64)
    st = np.full(1, -1, np.int32)
    assert emu.emu_frame_open_v1(_p(buf), C.c_uint64(len(frame)), n, C.c_uint64(f["content_bytes"]), 0, n, _p(in_off),
                             _p(out_off), _p(st)) == 0
    assert int(st[0]) == errno.EINVAL and not in_off.any() and not out_off.any()


# ---------------------------------------------------------------------------------- the decode kernels
def small_mixed_frame():
    """4 KB blocks: text, noise, text, noise, a ragged block of text -- stored and stream blocks side by side"""
    import oracle_lib as O
    text = O.corpus("laozi.txt")
    noise = W2.random_bytes(8192, 5)
    data = text[:4096] + noise[:4096] + text[4096:8192] + noise[4096:] + text[8192:9000]
    frame = W2.write_frame(data, 12, 12)
    assert [b["stored"] for b in W2.blocks(frame)] == [0, 1, 0, 1, 0]
    return data, frame


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_decode_under_the_mask(emu, waves):
    data, frame = small_mixed_frame()
    f = W2.fields(frame)
    n, content = f["n_blocks"], f["content_bytes"]
    for first, n_sel in ((0, n), (1, 2), (3, 2)):
        buf = aligned_copy(frame)
        lo, hi = first * 4096, min((first + n_sel) * 4096, content)
        in_off, out_off = np.zeros(n_sel + 1, np.uint64), np.zeros(n_sel + 1, np.uint64)
        stored, st = np.zeros(n_sel + 1, np.uint32), np.full(1, -1, np.int32)
        out = np.full(hi - lo + GUARD, 0xA5, np.uint8)
        toks = np.full(hi - lo + 64, 0xDEADBEEF, np.uint32)
        cnt, err = np.full(n_sel, 0xDEADBEEF, np.uint32), np.full(n_sel, -1, np.int32)
        rc = emu.emu_frame_decode_v2(_p(buf), C.c_uint64(len(frame)), n, C.c_uint64(content), first, n_sel, _p(in_off),
                                     _p(out_off), _p(stored), _p(st), _p(out), _p(toks), _p(cnt), _p(err), waves)
        assert rc == 0 and int(st[0]) == 0 and not err.any()
        assert out[:hi - lo].tobytes() == data[lo:hi] and (out[hi - lo:] == 0xA5).all()
        for k in range(n_sel):
            a, b = int(out_off[k]), int(out_off[k + 1])
            if stored[k]:                                    # a stored block: no tokens, its slots untouched
                assert cnt[k] == 0 and (toks[a:b] == 0xDEADBEEF).all()
            else:
                assert cnt[k] > 0


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_skip_mask_leaves_marked_blocks_alone(emu, waves):
    """the decode kernels alone: a marked block's input is never read (its range here is garbage), its output and
    token slots stay as they were; a null mask is the decoder as it always was"""
    import oracle_lib as O
    text = O.corpus("laozi.txt")
    blocks = [text[:3000], text[3000:7000], text[7000:7100], text[7100:9000]]
    streams = [O.encode(b, 12, header=False) for b in blocks]
    sizes = [len(b) for b in blocks]
    out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    for skip in (None, [0, 1, 0, 1], [1, 1, 1, 1]):
        parts = [s if not (skip and skip[k]) else b"\xFF" * len(s) for k, s in enumerate(streams)]
        data = np.frombuffer(b"".join(parts) + bytes(16), np.uint8).copy()
        in_off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.uint64)
        out = np.full(int(out_off[-1]) + 8, 0xA5, np.uint8)
        toks = np.full(int(out_off[-1]) + 64, 0xDEADBEEF, np.uint32)
        cnt, err = np.full(4, 0xDEADBEEF, np.uint32), np.full(4, -1, np.int32)
        m = None if skip is None else np.asarray(skip, np.uint32)
        emu.emu_decode_skip(_p(data), _p(in_off), 4, _p(out), _p(out_off), _p(toks), _p(cnt), _p(err), waves, _p(m))
        assert not err.any()
        for k in range(4):
            a, b = int(out_off[k]), int(out_off[k + 1])
            if skip and skip[k]:
                assert cnt[k] == 0 and (out[a:b] == 0xA5).all() and (toks[a:b] == 0xDEADBEEF).all(), (skip, k)
            else:
                assert out[a:b].tobytes() == blocks[k], (skip, k)
