"""CPU: the kernels of a batch of frames (sqz_amd/csrc/frame.hip, "batches of frames") -- the scans, the plan, the index
with its seal, the open and the verify for k frames -- compiled by g++ against tests/emu/hip/hip_runtime.h, each run by
itself lane by lane on the CPU wave emulator with guard values behind every array, and held against the independent
writers (tests/frame_writer*.py) and formulas written out here.  This pins the kernels' LOGIC without a GPU; the -m gpu
tests pin the gfx950 build."""
import ctypes as C
import errno
import functools
import os
import subprocess

import numpy as np
import pytest

import frame_gather_cases as G
import frame_writer as W
import frame_writer_v2 as W2
import frame_writer_v3 as W3
import frame_writer_v4 as W4
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
GUARD = 0xA5
G64, G32 = 0x7777777777777777, 0x77777777
STORED = 1
WB, BITS = 15, 12
BB = 1 << BITS
ITEM = np.dtype([("frame_at", "<u8"), ("avail", "<u8"), ("content_bytes", "<u8"), ("out_at", "<u8"),
                 ("n_blocks", "<u4"), ("zero", "<u4")])


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU, "libsqz_emu_frames.so")
    deps = [os.path.join(EMU, f) for f in ("emu_runtime.cpp", "emu_frames.cpp", "hip/hip_runtime.h")] + \
           [os.path.join(CSRC, f) for f in ("frame.hip", "sqz_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-I" + EMU,
                               "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                               "-Wno-attributes", os.path.join(EMU, "emu_runtime.cpp"),
                               os.path.join(EMU, "emu_frames.cpp"), "-o", out])
    return C.CDLL(out)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def aligned(n, fill=GUARD):
    raw = np.full(n + 16, fill, np.uint8)
    return raw[(-raw.ctypes.data) % 16:][:n]


# ---------------------------------------------------------------------------------- the formulas, written out
def pad8(n):
    return (n + 7) & ~7


def pad16(n):
    return (n + 15) & ~15


def blocks_in(c, bits=BITS):
    return (c + (1 << bits) - 1) >> bits


def sqz_bound(n):
    return (2 * n + 1024 + 7) & ~7


def frame_bound(c, bits, store):
    bb = 1 << bits
    off = pad16(32 + 8 * blocks_in(c, bits))
    if store:
        return off + pad8(c)
    return off + (c // bb) * sqz_bound(bb) + (sqz_bound(c % bb) if c % bb else 0)


def layout(sizes, bits, store):
    """(in_at, frame_at, base): k + 1 entries each"""
    in_at, frame_at, base = [0], [0], [0]
    for c in sizes:
        in_at.append(in_at[-1] + c)
        frame_at.append(frame_at[-1] + pad16(frame_bound(c, bits, store)))
        base.append(base[-1] + blocks_in(c, bits))
    return in_at, frame_at, base


# ---------------------------------------------------------------------------------- contents
@functools.lru_cache(maxsize=None)
def content(name):
    if name in G.PATTERNS:
        return G.content(name)
    return {"empty": b"", "one": b"q", "block": G.piece("c"),
            "ragged1": G.piece("a") + b"x",                   # a last block of 1 byte
            "ragged4095": G.piece("d") + G.piece("e")[:BB - 1],     # and of block - 1 bytes
            "noise": W2.random_bytes(2 * BB + 77, 5)}[name]


@functools.lru_cache(maxsize=None)
def streams(name):
    if name in G.PATTERNS:
        return tuple(G._stream(c, 1, False) for c in G.PATTERNS[name])
    return tuple(O.encode(b, WB, header=False) for b in W.blocks_of(content(name), BITS))


@functools.lru_cache(maxsize=None)
def frame(name, version):
    asm = W.assemble if version == 1 else W2.assemble
    return asm(content(name), WB, BITS, list(streams(name)))


SMALL = ("empty", "one", "block", "ragged1", "mixed", "ragged4095", "whole", "short", "noise")
BATCHES = {
    1: ("mixed",),
    2: ("b70", "empty"),
    5: ("ragged1", "b300", "empty", "noise", "ragged4095"),
    70: tuple(["b70"] + [SMALL[j % len(SMALL)] for j in range(68)] + ["one"]),
}


def test_the_contents_have_the_block_counts_the_batches_are_about():
    assert [blocks_in(len(content(n))) for n in ("empty", "one", "mixed", "b70", "b300")] == [0, 1, 3, 70, 300]
    assert len(content("ragged1")) % BB == 1 and len(content("ragged4095")) % BB == BB - 1
    assert sorted(BATCHES) == [1, 2, 5, 70] and all(len(v) == k for k, v in BATCHES.items())
    assert any(b["stored"] for b in W2.blocks(frame("noise", 2))) and any(b["stored"] for b in W2.blocks(frame("mixed", 2)))


# ---------------------------------------------------------------------------------- encode: scan and plan
@pytest.mark.parametrize("store", [False, True])
def test_encode_scan_and_plan_lay_out_the_batch(emu, store):
    rng = np.random.default_rng(3)
    lists = [[len(content(n)) for n in names] for names in BATCHES.values()]
    lists.append([int(v) for v in rng.integers(0, 9 * BB, 600)])      # more frames than lanes: shares of three
    lists.append([0, 0, 0])
    for bits in (12, 13):
        for sizes in lists:
            k = len(sizes)
            in_at, frame_at, base = layout(sizes, bits, store)
            c = np.asarray(sizes + [G64], np.uint64)
            a, b, d = np.full(k + 2, G64, np.uint64), np.full(k + 2, G64, np.uint64), np.full(k + 2, G32, np.uint32)
            emu.emu_frames_encode_scan(_p(c), k, bits, STORED if store else 0, _p(a), _p(b), _p(d))
            assert a.tolist() == in_at + [G64] and b.tolist() == frame_at + [G64] and d.tolist() == base + [G32]
            total, slab = base[-1], sqz_bound(1 << bits)
            in_off, slab_off = np.full(total + 2, G64, np.uint64), np.full(total + 2, G64, np.uint64)
            emu.emu_frames_plan(_p(c), _p(a), _p(d), k, bits, C.c_uint64(slab), _p(in_off), _p(slab_off))
            want = [in_at[f] + (j << bits) for f in range(k) for j in range(blocks_in(sizes[f], bits))] + [in_at[-1]]
            assert in_off.tolist() == want + [G64]
            assert slab_off.tolist() == [g * slab for g in range(total + 1)] + [G64]


# ---------------------------------------------------------------------------------- encode: index and seal
def run_index(em, names, store, fail=None):
    """fail: (frame, block, errno) -- a block the encoder failed"""
    k = len(names)
    sizes = [len(content(n)) for n in names]
    in_at, frame_at, base = layout(sizes, BITS, store)
    total = base[-1]
    out_bytes = np.asarray([len(s) for n in names for s in streams(n)] + [G64], np.uint64)
    crcs = np.asarray([b["content_crc"] for n in names for b in W2.blocks(frame(n, 1))] + [G32], np.uint32)
    err = np.zeros(total + 1, np.int32)
    if fail is not None:
        err[base[fail[0]] + fail[1]] = fail[2]
    buf = aligned(frame_at[-1] + 64)
    copy_bytes, dense_off = np.full(total + 1, G64, np.uint64), np.full(total + 2, G64, np.uint64)
    dense_rel = np.full(total + k + 1, G64, np.uint64)
    stored = np.full(total + 1, G32, np.uint32)
    fb, st = np.full(k + 1, G64, np.uint64), np.full(k + 1, -7, np.int32)
    em.emu_frames_index(_p(out_bytes), _p(err), _p(crcs), _p(np.asarray(sizes + [G64], np.uint64)),
                        _p(np.asarray(frame_at, np.uint64)), _p(np.asarray(base, np.uint32)), k, WB, BITS,
                        STORED if store else 0, _p(buf), _p(copy_bytes), _p(dense_rel), _p(dense_off),
                        _p(stored) if store else None, _p(fb), _p(st))
    assert copy_bytes[total] == G64 and dense_off[total + 1] == G64 and dense_rel[total + k] == G64
    assert stored[total] == G32 and fb[k] == G64 and st[k] == -7
    if not store:
        assert (stored == G32).all()
    return frame_at, base, buf, copy_bytes, dense_off, stored, fb, st


def check_index(names, store, result, failed=()):
    frame_at, base, buf, copy_bytes, dense_off, stored, fb, st = result
    version = 2 if store else 1
    for f, name in enumerate(names):
        want = frame(name, version)
        blk = W2.blocks(want)
        g0, n = base[f], len(blk)
        slot = buf[frame_at[f]:frame_at[f + 1]]
        assert int(fb[f]) == len(want)                                      # the size needed is reported either way
        if f in failed:
            assert (slot == GUARD).all() and not copy_bytes[g0:g0 + n].any() and not dense_off[g0:g0 + n].any()
            assert not store or not stored[g0:g0 + n].any()
            continue
        off = W.fields(want)["payload_off"]
        assert int(st[f]) == 0
        assert slot[:off].tobytes() == want[:off], (name, f)
        assert (slot[off:] == GUARD).all()                                  # the payload is other kernels' business
        assert dense_off[g0:g0 + n].tolist() == [frame_at[f] + b["payload_off"] for b in blk]
        assert copy_bytes[g0:g0 + n].tolist() == [0 if b["stored"] else len(s) for b, s in zip(blk, streams(name))]
        if store:
            assert stored[g0:g0 + n].tolist() == [b["stored"] for b in blk]
    last = len(names) - 1
    assert int(dense_off[base[-1]]) == (0 if last in failed else frame_at[last] + len(frame(names[last], version)))
    assert (buf[frame_at[-1]:] == GUARD).all()


@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("k", sorted(BATCHES))
def test_index_kernel_writes_the_writers_headers_indexes_and_dense_offsets(emu, k, store):
    check_index(BATCHES[k], store, run_index(emu, BATCHES[k], store))


@pytest.mark.parametrize("store", [False, True])
def test_a_frame_with_a_failed_block_writes_nothing_and_leaves_the_others_whole(emu, store):
    names = BATCHES[5]
    for f, b in ((1, 299), (0, 0), (4, 1)):                   # a middle frame, the first and the last one
        result = run_index(emu, names, store, fail=(f, b, errno.EIO))
        assert int(result[7][f]) == errno.EIO
        check_index(names, store, result, failed=(f,))
    sizes = np.asarray([16, G64], np.uint64)                   # a stream size no index entry holds
    _, frame_at, base = layout([len(content("one"))], BITS, store)
    buf = aligned(frame_at[-1])
    out_bytes, crcs, err = np.asarray([12], np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.int32)
    cb, do, dr = np.zeros(1, np.uint64), np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    sm, fb, st = np.zeros(1, np.uint32), np.zeros(1, np.uint64), np.zeros(1, np.int32)
    emu.emu_frames_index(_p(out_bytes), _p(err), _p(crcs), _p(np.asarray([1], np.uint64)),
                         _p(np.asarray(frame_at, np.uint64)), _p(np.asarray(base, np.uint32)), 1, WB, BITS,
                         STORED if store else 0, _p(buf), _p(cb), _p(dr), _p(do), _p(sm) if store else None, _p(fb), _p(st))
    assert int(st[0]) == errno.EINVAL and (buf == GUARD).all()


def test_a_batch_with_the_stored_flag_marks_exactly_the_blocks_the_writer_stores(emu):
    names = ("noise", "mixed", "b70")
    _, base, _, _, _, stored, _, _ = run_index(emu, names, True)
    want = [b["stored"] for n in names for b in W2.blocks(frame(n, 2))]
    assert stored[:base[-1]].tolist() == want and 0 < sum(want) < len(want)


# ---------------------------------------------------------------------------------- decode: scan, open, verify
@functools.lru_cache(maxsize=None)
def other_frame(version):
    """frames with another window and 8 KB blocks (a ragged last one), one of either version"""
    data = G.content("whole") + G.piece("N")[:1000] + G.piece("b")[:333]
    if version == 1:
        return data, W.write_frame(data, 12, 13)
    return data, W2.write_frame(data, 12, 13)


def lay_frames(frames, gaps=True):
    """frames: [(frame bytes, n_blocks, content_bytes)] -> (buffer, items, base, out_at): frames at multiples of 16 with
    guard bytes between them, outputs with gaps of 5, 10, ... bytes"""
    k = len(frames)
    items = np.zeros(k + 1, ITEM)
    at, out = 0, 100
    for f, (fr, n, c) in enumerate(frames):
        items[f] = (at, len(fr), c, out, n, 0)
        at += pad16(len(fr)) + (16 * (f % 3) if gaps else 0)
        out += c + (5 * (f + 1) if gaps else 0)
    buf = aligned(at + 32)
    for f, (fr, n, c) in enumerate(frames):
        a = int(items[f]["frame_at"])
        buf[a:a + len(fr)] = np.frombuffer(fr, np.uint8)
    items[k] = (G64, G64, G64, G64, G32, G32)
    base = np.cumsum([0] + [n for _, n, _ in frames]).tolist()
    return buf, items, base


def run_open(em, frames, gaps=True, avail=None):
    k = len(frames)
    buf, items, base = lay_frames(frames, gaps)
    if avail is not None:
        items[avail[0]]["avail"] = avail[1]
    got_base = np.full(k + 2, G32, np.uint32)
    em.emu_frames_decode_scan(_p(items), k, _p(got_base))
    assert got_base.tolist() == base + [G32]
    entries = base[-1] + k
    in_off, out_off = np.full(entries + 2, G64, np.uint64), np.full(entries + 2, G64, np.uint64)
    skip, stored = np.full(entries + 1, G32, np.uint32), np.full(entries + 1, G32, np.uint32)
    st = np.full(k + 1, -7, np.int32)
    out_base = int(items[0]["out_at"])
    em.emu_frames_open(_p(buf), _p(items), _p(got_base), k, C.c_uint64(out_base), _p(in_off), _p(out_off), _p(skip),
                       _p(stored), _p(st))
    assert in_off[entries + 1] == G64 and out_off[entries + 1] == G64 and skip[entries] == G32 and stored[entries] == G32
    assert st[k] == -7
    return items, base, in_off, out_off, skip, stored, st


def entries_of(items, base, f, fr, refused=False):
    """what frame f's n + 1 entries hold: (in_off, out_off, skip, stored)"""
    at, to = int(items[f]["frame_at"]), int(items[f]["out_at"]) - int(items[0]["out_at"])
    n = int(items[f]["n_blocks"])
    if refused:
        return [at] * (n + 1), [to] * (n + 1), [1] * (n + 1), [0] * (n + 1)
    fl, blk = W.fields(fr), W2.blocks(fr)
    ins = [at + b["payload_off"] for b in blk] + [at + len(fr)]
    outs = [to + min(j * fl["block_bytes"], fl["content_bytes"]) for j in range(n + 1)]
    return ins, outs, [b["stored"] for b in blk] + [1], [b["stored"] for b in blk] + [0]


def check_open(frames, result, want_status):
    items, base, in_off, out_off, skip, stored, st = result
    for f, (fr, n, c) in enumerate(frames):
        e0 = base[f] + f
        assert int(st[f]) == want_status[f], f
        ins, outs, sk, sd = entries_of(items, base, f, fr, refused=want_status[f] != 0)
        assert in_off[e0:e0 + n + 1].tolist() == ins and out_off[e0:e0 + n + 1].tolist() == outs, f
        assert skip[e0:e0 + n + 1].tolist() == sk and stored[e0:e0 + n + 1].tolist() == sd, f
    end = base[-1] + len(frames)
    assert in_off[end] == in_off[end - 1] and out_off[end] == out_off[end - 1]


def triple(fr, data):
    return fr, W.fields(fr)["n_blocks"], len(data)


def mixed_batch():
    d1, f1 = other_frame(1)
    d2, f2 = other_frame(2)
    return [triple(frame("mixed", 2), content("mixed")), triple(f1, d1), triple(frame("empty", 1), b""),
            triple(frame("short", 1), content("short")), triple(f2, d2), triple(frame("ragged1", 2), content("ragged1"))]


def test_open_kernel_lays_out_a_mixed_batch_of_versions_and_block_sizes(emu):
    frames = mixed_batch()
    assert {W.fields(f)["block_bytes"] for f, _, _ in frames} == {4096, 8192}
    assert {W.fields(f)["version"] for f, _, _ in frames} == {1, 2}
    for gaps in (True, False):
        check_open(frames, run_open(emu, frames, gaps), [0] * len(frames))


@pytest.mark.parametrize("k", sorted(BATCHES))
def test_open_kernel_at_every_batch_shape(emu, k):
    frames = [triple(frame(n, 1 + (j % 2)), content(n)) for j, n in enumerate(BATCHES[k])]
    check_open(frames, run_open(emu, frames), [0] * k)


def test_every_malformed_variant_costs_its_frame_alone(emu):
    before, behind = triple(frame("whole", 2), content("whole")), triple(frame("short", 1), content("short"))
    # what a caller's table holds: the header's own figures where the header alone parses, the good frame's otherwise
    variants = [(name, bad, want if head == 0 else errno.EINVAL,
                 W.fields(bad)["content_bytes"] if head == 0 else len(content("mixed")))
                for version, R in ((1, W.refusals), (2, W2.refusals))
                for name, bad, head, want in R(frame("mixed", version))]
    variants.append(("version_3", G.frame("mixed", 3), errno.EINVAL, len(G.content("mixed"))))
    data4 = W4.figure_input("u32_ramp")
    variants.append(("version_4", W4.write_frame(data4, WB, BITS, 4), errno.EINVAL, len(data4)))
    variants.append(("version_4_stored", W4.write_frame(data4, WB, BITS, 4, True), errno.EINVAL, len(data4)))
    assert len(variants) == 12 + 9 + 3
    for name, bad, want, size in variants:
        frames = [before, (bad, blocks_in(size), size), behind]
        check_open(frames, run_open(emu, frames), [0, want, 0])
    # what the table says and the header does not; a payload that avail does not cover
    good = frame("mixed", 1)
    for mid, want in (((good, 3, len(content("mixed")) - 1), errno.EINVAL), ((good, 2, len(content("mixed"))), errno.EINVAL)):
        frames = [before, mid, behind]
        check_open(frames, run_open(emu, frames), [0, want, 0])
    frames = [before, triple(good, content("mixed")), behind]
    check_open(frames, run_open(emu, frames, avail=(1, len(good) - 8)), [0, errno.E2BIG, 0])
    # a refused first and a refused last frame
    bad = W.refusals(good)[0][1]
    frames = [triple(bad, content("mixed")), before, triple(bad, content("mixed"))]
    check_open(frames, run_open(emu, frames), [errno.EINVAL, 0, errno.EINVAL])


def test_verify_kernel_gives_every_block_its_errno(emu):
    frames = mixed_batch() + [triple(frame("b300", 2), content("b300"))]
    k = len(frames)
    buf, items, base = lay_frames(frames)
    entries, total = base[-1] + k, base[-1]
    crc, err = np.full(entries + 1, 0x1234567, np.uint32), np.zeros(entries + 1, np.int32)
    for f, (fr, n, c) in enumerate(frames):
        crc[base[f] + f:base[f] + f + n] = [b["content_crc"] for b in W2.blocks(fr)]
    status = np.zeros(k + 1, np.int32)
    status[3] = errno.EILSEQ                                                 # a refused frame: its status everywhere
    want = np.zeros(total, np.int32)
    want[base[3]:base[4]] = errno.EILSEQ
    crc[base[0] + 0 + 1] ^= 1                                                # frame 0, block 1: the bytes are not the ones
    want[base[0] + 1] = errno.EILSEQ
    err[base[6] + 6 + 299] = errno.EINVAL                                    # the decoder's own errno is kept
    want[base[6] + 299] = errno.EINVAL
    crc[base[6] + 6 + 299] ^= 4
    err[base[4] + 4 + 0] = errno.EIO
    want[base[4] + 0] = errno.EIO
    crc[base[3] + 3] ^= 1                                                    # (refused: not looked at)
    out = np.full(total + 1, -7, np.int32)
    emu.emu_frames_verify(_p(buf), _p(items), _p(np.asarray(base, np.uint32)), k, _p(crc), _p(status), _p(err), _p(out))
    assert out[:total].tolist() == want.tolist() and out[total] == -7
