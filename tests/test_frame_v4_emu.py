"""CPU: the kernels of SQZF version 4 -- the byte shuffle (sqz_amd/csrc/shuffle.hip) and the version-4 flavours of the
index and open kernels (sqz_amd/csrc/frame.hip) -- compiled by g++ against tests/emu/hip/hip_runtime.h, run lane by
lane on the CPU wave emulator and held against numpy and the independent writer (tests/frame_writer_v4.py).  This pins
the kernels' LOGIC, every alignment and every byte they may not touch, without a GPU; the -m gpu tests pin the gfx950
build."""
import ctypes as C
import errno
import os
import subprocess

import numpy as np
import pytest

import frame_writer_v4 as W4
from test_frame_emu import LENGTHS, aligned_copy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
TILE_BYTES = 8192                                            # kShufTile: a tile is TILE_BYTES / e elements
GUARD = 0xA5


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU, "libsqz_emu_frame_v4.so")
    deps = [os.path.join(EMU, f) for f in ("emu_runtime.cpp", "emu_frame_v4.cpp", "hip/hip_runtime.h")] + \
           [os.path.join(CSRC, f) for f in ("frame.hip", "shuffle.hip", "sqz_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-I" + EMU,
                               "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                               "-Wno-attributes", os.path.join(EMU, "emu_runtime.cpp"),
                               os.path.join(EMU, "emu_frame_v4.cpp"), "-o", out])
    return C.CDLL(out)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def aligned(n, fill):
    raw = np.full(n + 16, fill, np.uint8)
    return raw[(-raw.ctypes.data) % 16:][:n]


def lengths_for(e):
    t = TILE_BYTES // e                                      # one below, at and above the tile, in elements
    tile = [(t - 1) * e, t * e, (t + 1) * e, t * e + e - 1]
    return sorted(set(LENGTHS + list(range(2 * e + 2)) + tile))


RNG = np.random.default_rng(11)
PATTERN = RNG.integers(0, 256, 160000, dtype=np.uint8)


def run(em, e, inverse, ranges, src_mis, dst_mis, hint=0, skip=None):
    """ranges: [(start, length)] ascending, not overlapping, relative to a base that is misaligned by src_mis in the
    source and by dst_mis in the destination; -> (source bytes, destination bytes) with the base at index 0"""
    end = max((s + n for s, n in ranges), default=0)
    src = aligned(end + 64, 0)
    dst = aligned(end + 64, GUARD)
    src[:] = PATTERN[:len(src)]
    sb, db = src[src_mis:], dst[dst_mis:]
    # one offsets array serves both sides: range b is [off[b], off[b + 1]); gaps between ranges are ranges to skip
    cuts, mask = [], []
    at = 0
    for s, n in ranges:
        if s > at:
            cuts.append(at)
            mask.append(1)
        cuts.append(s)
        mask.append(0)
        at = s + n
    cuts.append(at)
    if skip is not None:
        for k in skip:
            mask[k] = 1
    off = np.asarray(cuts, np.uint64)
    m = np.asarray(mask + [0], np.uint32)
    em.emu_shuffle_blocks(_p(sb), _p(off), len(cuts) - 1, e, int(inverse), _p(db), _p(m) if any(mask) else None,
                          C.c_uint64(hint))
    return sb, db, dst, list(zip(cuts, cuts[1:], mask))


def check(em, e, inverse, ranges, src_mis, dst_mis, hint=None):
    # hint: the launch's size hint, by default the largest range (a workgroup per 32 KB); 0 = unknown, which launches
    # the most workgroups a range, most of which leave at once (slow on the emulator: a few cases only)
    if hint is None:
        hint = max([n for _, n in ranges] + [1])
    sb, db, dst, cut = run(em, e, inverse, ranges, src_mis, dst_mis, hint)
    want = np.full(len(dst), GUARD, np.uint8)
    for a, b, masked in cut:
        if not masked:
            blk = sb[a:b].tobytes()
            got = W4.unshuffle(blk, e) if inverse else W4.shuffle(blk, e)
            want[dst_mis + a:dst_mis + b] = np.frombuffer(got, np.uint8)
    bad = np.nonzero(dst != want)[0]
    assert bad.size == 0, (e, inverse, ranges, src_mis, dst_mis, hint, bad[:8].tolist())


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("e", W4.ELEMS)
def test_shuffle_of_one_range_at_every_length(emu, e, inverse):
    for n in lengths_for(e):
        for mis in ((0, 0), (1, 0), (0, 1), (3, 9), (15, 2), (8, 8), (17, 16)):
            check(emu, e, inverse, [(0, n)], *mis)
        if n in (0, 1, 2 * e + 1, 4097, 70001):
            check(emu, e, inverse, [(0, n)], 5, 11, hint=0)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("e", W4.ELEMS)
def test_shuffle_at_every_pair_of_misalignments_between_guard_bytes(emu, e, inverse):
    t = TILE_BYTES // e
    for n in (2 * e + 1, 255, 4097, (t + 1) * e + 3):
        for s in range(18):
            for d in range(18):
                check(emu, e, inverse, [(0, n)], s, d)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("e", W4.ELEMS)
def test_shuffle_of_ragged_ranges_in_one_launch(emu, e, inverse):
    # neighbours that touch, an empty range among them, gaps that must stay untouched, a range of three tiles
    ranges = [(0, 5), (5, 4096), (4101, 0), (4101, 1), (4110, 3 * TILE_BYTES + 7 * e + 1), (30000, e - 1), (30010, 16389)]
    for mis in ((0, 0), (1, 7), (16, 3), (13, 13)):
        check(emu, e, inverse, ranges, *mis)
        check(emu, e, inverse, ranges, *mis, hint=TILE_BYTES)          # fewer workgroups than the longest range has tiles
    check(emu, e, inverse, ranges, 2, 5, hint=0)


def test_shuffle_of_more_ranges_than_the_launch_shares_workgroups_among(emu):
    many = [(17 * k, 17) for k in range(8200)]               # one workgroup a range
    check(emu, 4, False, many, 3, 6)
    check(emu, 2, True, many, 6, 3)


@pytest.mark.parametrize("e", W4.ELEMS)
def test_a_skipped_range_is_left_alone_and_the_round_trip_is_the_identity(emu, e):
    sb, db, dst, cut = run(emu, e, False, [(0, 4097), (4097, 300), (4397, 9000)], 1, 2, skip=[1])
    assert (db[4097:4397] == GUARD).all() and db[:4097].tobytes() == W4.shuffle(sb[:4097].tobytes(), e)
    for n in (4096, 16389):
        data = PATTERN[:n].copy()
        mid, back = aligned(n + 32, GUARD), aligned(n + 32, GUARD)
        off = np.asarray([0, n], np.uint64)
        emu.emu_shuffle_blocks(_p(data), _p(off), 1, e, 0, _p(mid), None, C.c_uint64(n))
        emu.emu_shuffle_blocks(_p(mid), _p(off), 1, e, 1, _p(back), None, C.c_uint64(n))
        assert back[:n].tobytes() == data.tobytes() and (back[n:] == GUARD).all()


# ---------------------------------------------------------------------------------- index and open
def content():
    return W4.figure_input("u32_ramp")                       # 16389 bytes: four blocks of 4 KB and a ragged one of 5


def noise():
    return W4.figure_input("u32_noise")


def run_index(em, data, e, store, capacity=None, err=None, flags=None):
    frame = W4.write_frame(data, 15, 12, e, store)
    f, blk = W4.fields(frame), W4.blocks(frame)
    n = f["n_blocks"]
    sizes = np.asarray([len(s) for s in W4.streams_of(data, 15, 12, e)] + [0], np.uint64)
    crcs = np.asarray([b["content_crc"] for b in blk] + [0], np.uint32)
    out = aligned(len(frame) + 64, GUARD)
    err_a = np.zeros(n + 1, np.int32) if err is None else np.asarray(err, np.int32)
    copy_bytes, dense_off = np.full(n + 1, 77, np.uint64), np.full(n + 2, 77, np.uint64)
    stored = np.full(n + 1, 77, np.uint32)
    fb, st = np.zeros(1, np.uint64), np.full(1, -1, np.int32)
    # SQZ_FRAME_SHUFFLE is set in the header with or without the bit in the call's flags
    flags = (W4.STORED if store else 0) | (W4.SHUFFLE if flags is None else flags)
    em.emu_frame_index_v4(_p(sizes), _p(err_a), _p(crcs), n, C.c_uint64(len(data)), 15, 12, flags, e, _p(out),
                          C.c_uint64(len(frame) if capacity is None else capacity), _p(copy_bytes), _p(dense_off),
                          _p(stored), _p(fb), _p(st))
    return frame, f, blk, sizes[:n], out, copy_bytes, dense_off, stored, int(fb[0]), int(st[0])


@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("e", W4.ELEMS)
def test_index_kernel_writes_the_writers_header_index_record_and_work_lists(emu, e, store):
    for data in (content(), noise(), content()[:4096], content()[:8192], b""):
        for flags in (None, 0):
            frame, f, blk, sizes, out, copy_bytes, dense_off, stored, fb, st = run_index(emu, data, e, store, flags=flags)
            n = f["n_blocks"]
            assert st == 0 and fb == len(frame)
            assert out[:f["payload_off"]].tobytes() == frame[:f["payload_off"]]
            assert (out[f["payload_off"]:] == GUARD).all()                  # the payload is other kernels' business
            assert dense_off[:n + 1].tolist() == [b["payload_off"] for b in blk] + [len(frame)]
            assert copy_bytes[:n].tolist() == [0 if b["stored"] else int(s) for b, s in zip(blk, sizes)]
            if store:
                assert stored[:n].tolist() == [b["stored"] for b in blk]
            assert copy_bytes[n] == 77 and dense_off[n + 1] == 77 and stored[n] == 77
    assert all(b["stored"] for b in W4.blocks(W4.write_frame(noise(), 15, 12, 4, True)))


def test_index_kernel_refuses_without_writing(emu):
    data = content()
    size = len(W4.write_frame(data, 15, 12, 2, True))
    for kw, want in (({"capacity": size - 8}, errno.E2BIG), ({"err": [0, 0, errno.EIO, 0, 0, 0]}, errno.EIO)):
        frame, f, blk, sizes, out, copy_bytes, dense_off, stored, fb, st = run_index(emu, data, 2, True, **kw)
        n = f["n_blocks"]
        assert st == want and fb == size                                    # the size needed is still reported
        assert (out == GUARD).all() and not copy_bytes[:n].any() and not dense_off[:n + 1].any() and not stored[:n].any()


def run_open(em, frame, n, content_bytes, e, first=0, n_sel=None, avail=None, want_bits=0):
    n_sel = n - first if n_sel is None else n_sel
    buf = aligned_copy(frame)
    in_off, out_off = np.full(n_sel + 2, 99, np.uint64), np.full(n_sel + 2, 99, np.uint64)
    stored = np.full(n_sel + 1, 99, np.uint32)
    st = np.full(1, -1, np.int32)
    rc = em.emu_frame_open_v4(_p(buf), C.c_uint64(len(frame) if avail is None else avail), n, C.c_uint64(content_bytes),
                              first, n_sel, e, _p(in_off), _p(out_off), _p(stored), _p(st), want_bits)
    assert stored[n_sel] == 99 and in_off[n_sel + 1] == 99 and out_off[n_sel + 1] == 99
    return rc, int(st[0]), in_off[:n_sel + 1].tolist(), out_off[:n_sel + 1].tolist(), stored[:n_sel].tolist()


@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("e", W4.ELEMS)
def test_open_kernel_builds_offsets_and_mask(emu, e, store):
    for data in (content(), noise()):
        frame = W4.write_frame(data, 15, 12, e, store)
        f, blk = W4.fields(frame), W4.blocks(frame)
        n, size = f["n_blocks"], f["block_bytes"]
        starts = [b["payload_off"] for b in blk] + [len(frame)]
        for first, n_sel in ((0, n), (1, 2), (n - 1, 1), (2, 0)):
            rc, st, in_off, out_off, stored = run_open(emu, frame, n, len(data), e, first, n_sel)
            assert (rc, st) == (0, 0)
            assert in_off == starts[first:first + n_sel + 1]
            assert out_off == [min((first + k) * size, len(data)) - first * size for k in range(n_sel + 1)]
            assert stored == [b["stored"] for b in blk[first:first + n_sel]]
        assert run_open(emu, frame, n, len(data), e, want_bits=12)[1] == 0
        assert run_open(emu, frame, n, len(data), e, want_bits=13)[1] == errno.EINVAL


def refused(result, n_sel):
    rc, st, in_off, out_off, stored = result
    assert in_off == [0] * (n_sel + 1) and out_off == [0] * (n_sel + 1) and stored == [0] * n_sel
    return st


@pytest.mark.parametrize("e", W4.ELEMS)
def test_open_kernel_refuses_every_malformed_variant_and_selects_nothing(emu, e):
    data = content()
    frame = W4.write_frame(data, 15, 12, e)
    n = W4.fields(frame)["n_blocks"]
    for name, bad, _, want in W4.refusals(frame):
        assert refused(run_open(emu, bad, n, len(data), e), n) == want, name
    for other in W4.ELEMS:                                   # the caller's elem_bytes is not the record's
        if other != e:
            assert refused(run_open(emu, frame, n, len(data), other), n) == errno.EINVAL
    assert refused(run_open(emu, frame, n, len(data) - 1, e), n) == errno.EINVAL
    assert refused(run_open(emu, frame, n, len(data), e, avail=len(frame) - 8), n) == errno.E2BIG
    assert refused(run_open(emu, frame, n, len(data), e, first=n, n_sel=1), 1) == errno.EINVAL


def test_the_open_kernels_there_were_refuse_version_4(emu):
    data = content()
    for store in (False, True):
        frame = W4.write_frame(data, 15, 12, 4, store)
        n = W4.fields(frame)["n_blocks"]
        buf = aligned_copy(frame)
        in_off, out_off = np.full(n + 1, 99, np.uint64), np.full(n + 1, 99, np.uint64)
        stored, st = np.full(n, 99, np.uint32), np.full(1, -1, np.int32)
        assert emu.emu_frame_open_old(_p(buf), C.c_uint64(len(frame)), n, C.c_uint64(len(data)), 0, n, _p(in_off),
                                      _p(out_off), _p(stored), _p(st)) == 0
        assert int(st[0]) == errno.EINVAL and not in_off.any() and not out_off.any() and not stored.any()
