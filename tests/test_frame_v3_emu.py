"""CPU: SQZF version 3 in the device-resident flavour and the ranged read from a resident frame -- the version-3
kernels of the index and open code, the read plan (sqz_amd/csrc/frame.hip) and the decode kernels behind them
(decode.hip) -- compiled by g++ against tests/emu/hip/hip_runtime.h, run lane by lane on the CPU wave emulator and
held against the independent version-3 writer (tests/frame_writer_v3.py over tests/dict_model.py).  This pins the
kernels' LOGIC without a GPU; the -m gpu tests (test_frame_v3_gpu.py) pin the gfx950 build."""
import ctypes as C
import errno
import os
import struct
import subprocess

import numpy as np
import pytest

import frame_v3_cases as K
import frame_writer as W
import frame_writer_v2 as W2
import frame_writer_v3 as W3
from test_frame_emu import aligned_copy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
GUARD = 24
E = errno


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU, "libsqz_emu_frame_v3.so")
    deps = [os.path.join(EMU, f) for f in ("emu_runtime.cpp", "emu_frame_v3.cpp", "hip/hip_runtime.h")] + \
           [os.path.join(CSRC, f) for f in ("frame.hip", "decode.hip", "sqz_tree.h", "sqz_device.h", "sqz_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-I" + EMU,
                               "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                               "-Wno-attributes", os.path.join(EMU, "emu_runtime.cpp"),
                               os.path.join(EMU, "emu_frame_v3.cpp"), "-o", out])
    return C.CDLL(out)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def aligned(n, fill):
    raw = np.full(n + 16, fill, np.uint8)
    return raw[(-raw.ctypes.data) % 16:][:n]


def _dict(d: bytes):
    return np.frombuffer(d + bytes(16), np.uint8).copy()


def test_the_shared_inputs_are_what_they_are_there_for():
    K.check_layout()


# ---------------------------------------------------------------------------------- the index kernel
def run_index(em, case, store, lazy, capacity=None, err=None):
    name, wb, bb, dct, data = case
    frame = K.frame(dct, data, wb, bb, store, lazy)
    f, blk = W3.fields(frame), W3.blocks(frame)
    n = f["n_blocks"]
    sizes = np.asarray([len(s) for s in K.streams(dct, data, wb, bb, lazy)] + [0], np.uint64)
    crcs = np.asarray([b["content_crc"] for b in blk] + [0], np.uint32)
    capacity = len(frame) if capacity is None else capacity
    out = aligned(len(frame) + 64, 0xA5)
    err_a = np.zeros(n + 1, np.int32) if err is None else np.asarray(err, np.int32)
    copy_bytes, dense_off = np.full(n + 1, 77, np.uint64), np.full(n + 2, 77, np.uint64)
    stored = np.full(n + 1, 77, np.uint32)
    fb, st = np.zeros(1, np.uint64), np.full(1, -1, np.int32)
    # SQZ_FRAME_DICT is set in the header with or without the bit in the call's flags
    flags = (W3.STORED if store else 0) | (0 if lazy else W3.DICT)
    d = _dict(dct)
    em.emu_frame_index_v3(_p(sizes), _p(err_a), _p(crcs), n, C.c_uint64(len(data)), wb, bb, flags, _p(d), len(dct),
                          _p(out), C.c_uint64(capacity), _p(copy_bytes), _p(dense_off), _p(stored), _p(fb), _p(st))
    return frame, f, blk, sizes[:n], out, copy_bytes, dense_off, stored, int(fb[0]), int(st[0])


@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("lazy", [False, True])
def test_index_kernel_writes_the_writers_header_index_record_and_work_lists(emu, store, lazy):
    for case in K.contents():
        frame, f, blk, sizes, out, copy_bytes, dense_off, stored, fb, st = run_index(emu, case, store, lazy)
        n, what = f["n_blocks"], (case[0], store, lazy)
        assert st == 0 and fb == len(frame), what
        assert f["payload_off"] == W3.pad16(32 + 8 * n + 8)
        assert out[:f["payload_off"]].tobytes() == frame[:f["payload_off"]], what
        assert (out[f["payload_off"]:] == 0xA5).all(), what                      # the payload is the copies'
        want_stored = [b["stored"] for b in blk]
        if store:
            assert stored[:n].tolist() == want_stored and stored[n] == 77, what
        else:
            assert not any(want_stored) and (stored == 77).all(), what           # no mask without SQZ_FRAME_STORED
        assert copy_bytes[:n].tolist() == [0 if s else int(v) for s, v in zip(want_stored, sizes)], what
        assert copy_bytes[n] == 77 and dense_off[n + 1] == 77, what
        assert dense_off[:n + 1].tolist() == [b["payload_off"] for b in blk] + [len(frame)], what


def test_index_kernel_refuses_without_writing(emu):
    case = [c for c in K.contents() if c[0] == "mixed"][0]
    size = len(K.frame(case[3], case[4], 15, 12, True, False))
    for kw, want in (({"capacity": size - 1}, E.E2BIG), ({"capacity": 0}, E.E2BIG), ({"err": [0, E.ENOBUFS, 0, 0]}, E.ENOBUFS)):
        frame, f, blk, sizes, out, copy_bytes, dense_off, stored, fb, st = run_index(emu, case, True, False, **kw)
        assert st == want and fb == size                             # the size needed is still reported
        assert (out == 0xA5).all() and not copy_bytes[:3].any() and not dense_off[:4].any() and not stored[:3].any()
        assert copy_bytes[3] == 77 and dense_off[4] == 77 and stored[3] == 77


# ---------------------------------------------------------------------------------- the open kernel
def run_open(em, frame, n, content, dct, first=0, n_sel=None, avail=None, want_bits=0):
    n_sel = n - first if n_sel is None else n_sel
    buf = aligned_copy(frame)
    in_off, out_off = np.full(n_sel + 2, 99, np.uint64), np.full(n_sel + 2, 99, np.uint64)
    stored = np.full(n_sel + 1, 99, np.uint32)
    st = np.full(1, -1, np.int32)
    d = _dict(dct)
    rc = em.emu_frame_open_v3(_p(buf), C.c_uint64(len(frame) if avail is None else avail), n, C.c_uint64(content), first,
                              n_sel, _p(d), len(dct), _p(in_off), _p(out_off), _p(stored), _p(st), want_bits)
    assert stored[n_sel] == 99 and in_off[n_sel + 1] == 99 and out_off[n_sel + 1] == 99
    return rc, int(st[0]), in_off[:n_sel + 1].tolist(), out_off[:n_sel + 1].tolist(), stored[:n_sel].tolist()


@pytest.mark.parametrize("store", [False, True])
def test_open_kernel_builds_offsets_and_mask(emu, store):
    for name, wb, bb, dct, data in K.contents():
        frame = K.frame(dct, data, wb, bb, store, False)
        f, blk = W3.fields(frame), W3.blocks(frame)
        n, size, content = f["n_blocks"], f["block_bytes"], f["content_bytes"]
        starts = [b["payload_off"] for b in blk] + [len(frame)]
        mask = [b["stored"] for b in blk]
        rc, st, in_off, out_off, stored = run_open(emu, frame, n, content, dct, want_bits=bb)
        assert (rc, st) == (0, 0), name
        assert in_off == starts and out_off == [min(k * size, content) for k in range(n + 1)] and stored == mask, name
        if n >= 3:
            for first, n_sel in ((1, 1), (n - 1, 1), (0, 2)):
                rc, st, in_off, out_off, stored = run_open(emu, frame, n, content, dct, first, n_sel)
                assert (rc, st) == (0, 0)
                assert in_off == starts[first:first + n_sel + 1] and stored == mask[first:first + n_sel]
                assert out_off == [min((first + k) * size, content) - first * size for k in range(n_sel + 1)]


def _refusals(store_frame, plain_frame, data, dct):
    """(name, frame, dictionary, what the caller passes as content_bytes, errno): each a good frame with ONE change,
    resealed where index_crc must hold for the check to be reached"""
    out = []
    n, content = 3, len(data)

    def put(name, at, fmt, value, want, reseal=False, base=store_frame, arg=content):
        b = bytearray(base)
        struct.pack_into(fmt, b, at, value)
        out.append((name, W3.reseal(b) if reseal else bytes(b), dct, arg, want))

    # 1: the header's own fields (whether index_crc holds or not)
    for reseal in (False, True):
        put("magic", 0, "<4s", b"SQZG", E.EINVAL, reseal)
        put("version_1", 4, "<B", 1, E.EINVAL, reseal)
        put("version_2", 4, "<B", 2, E.EINVAL, reseal)
        put("version_4", 4, "<B", 4, E.EINVAL, reseal)
        put("flags_without_bit_1", 7, "<B", W3.STORED, E.EINVAL, reseal)
        put("flags_none", 7, "<B", 0, E.EINVAL, reseal)
        put("flags_bit_2", 7, "<B", W3.DICT | W3.STORED | 4, E.EINVAL, reseal)
        put("flags_bit_7", 7, "<B", W3.DICT | 0x80, E.EINVAL, reseal)
        put("win_bits_9", 5, "<B", 9, E.EINVAL, reseal)
        put("win_bits_16", 5, "<B", 16, E.EINVAL, reseal)
        put("block_bits_11", 6, "<B", 11, E.EINVAL, reseal)
        put("block_bits_25", 6, "<B", 25, E.EINVAL, reseal)
        # 2: the header against the arguments
        put("n_blocks_plus_one", 24, "<I", n + 1, E.EINVAL, reseal)
        put("n_blocks_minus_one", 24, "<I", n - 1, E.EINVAL, reseal)
        put("content_bytes_is_not_the_callers", 8, "<Q", content - 1, E.EINVAL, reseal)
        put("block_bits_13", 6, "<B", 13, E.EINVAL, reseal)          # n_blocks no longer is ceil(content / block)
    out.append(("version_1_frame", W.write_frame(data, 15, 12), dct, content, E.EINVAL))
    out.append(("version_2_frame", W2.write_frame(data, 15, 12), dct, content, E.EINVAL))
    # 3: index_crc over [0, 28), the index and the record
    put("content_bytes_changed", 8, "<Q", content - 1, E.EILSEQ, arg=content - 1)
    put("index_bit_flipped", 32 + 8 + 5, "<B", store_frame[32 + 8 + 5] ^ 0x10, E.EILSEQ)
    put("record_length_flipped", 32 + 8 * n, "<B", store_frame[32 + 8 * n] ^ 1, E.EILSEQ)
    put("record_crc_flipped", 32 + 8 * n + 7, "<B", store_frame[32 + 8 * n + 7] ^ 0x80, E.EILSEQ)
    # 4: the record's dict_bytes
    put("record_dict_bytes_0", 32 + 8 * n, "<I", 0, E.EINVAL, True)
    put("record_dict_bytes_window", 32 + 8 * n, "<I", 1 << 15, E.EINVAL, True)
    # 5: a stored entry of the right size in a frame without bit 0 (payload_bytes adjusted: only the flag is missing)
    b = bytearray(plain_frame)
    words = struct.unpack_from("<I", b, 32)[0]
    struct.pack_into("<I", b, 32, 512 | W3.STORED_BIT)
    struct.pack_into("<Q", b, 16, struct.unpack_from("<Q", b, 16)[0] + 8 * (512 - words))
    out.append(("stored_entry_without_bit_0", W3.reseal(b), dct, content, E.EINVAL))
    #    and a stored entry that is not its block's size (the sum still is payload_bytes)
    b = bytearray(store_frame)
    struct.pack_into("<I", b, 32 + 8, 513 | W3.STORED_BIT)
    struct.pack_into("<Q", b, 16, struct.unpack_from("<Q", b, 16)[0] + 8)
    out.append(("stored_entry_of_another_size", W3.reseal(b), dct, content, E.EINVAL))
    # 6: the words do not sum to payload_bytes
    put("stream_words_sum", 32, "<I", struct.unpack_from("<I", store_frame, 32)[0] + 1, E.EINVAL, True)
    put("payload_bytes_odd", 16, "<Q", struct.unpack_from("<Q", store_frame, 16)[0] + 4, E.EINVAL, True)
    # 7: a good frame, another dictionary
    out.append(("dictionary_one_bit_off", store_frame, bytes([dct[0] ^ 1]) + dct[1:], content, E.EILSEQ))
    out.append(("dictionary_one_byte_shorter", store_frame, dct[:-1], content, E.EILSEQ))
    out.append(("dictionary_one_byte_longer", store_frame, dct + b"x", content, E.EILSEQ))
    return out


def test_open_kernel_refusals_in_the_hosts_order(emu):
    dct, data = K.dct(), K.mixed()
    store_frame, plain_frame = K.frame(dct, data, 15, 12, True, False), K.frame(dct, data, 15, 12, False, False)
    seen = set()
    for what, bad, d, content, want in _refusals(store_frame, plain_frame, data, dct):
        rc, st, in_off, out_off, stored = run_open(emu, bad, 3, content, d)
        assert (rc, st) == (0, want), (what, st)
        assert not any(in_off) and not any(out_off) and not any(stored), what   # zero-length ranges, nothing marked
        seen.add(want)
    assert seen == {E.EINVAL, E.EILSEQ}
    # 8: the payload beyond avail
    rc, st, in_off, out_off, stored = run_open(emu, store_frame, 3, len(data), dct, avail=len(store_frame) - 8)
    assert (rc, st) == (0, E.E2BIG) and not any(in_off) and not any(out_off) and not any(stored)
    # ... which a wrong dictionary comes before, and a bad sum before that
    rc, st, *_ = run_open(emu, store_frame, 3, len(data), dct[:-1], avail=len(store_frame) - 8)
    assert (rc, st) == (0, E.EILSEQ)
    # the selection leaves the frame; the caller's block_bits is not the frame's
    rc, st, in_off, out_off, stored = run_open(emu, store_frame, 3, len(data), dct, first=2, n_sel=2)
    assert (rc, st) == (0, E.EINVAL) and not any(in_off) and not any(stored)
    rc, st, in_off, out_off, stored = run_open(emu, store_frame, 3, len(data), dct, want_bits=13)
    assert (rc, st) == (0, E.EINVAL) and not any(in_off) and not any(stored)
    # a one-block frame reads the same at 12 and 13 bits by the arithmetic alone: want_bits is what notices
    one = K.frame(dct, data[:4096], 15, 12, False, False)
    assert run_open(emu, one, 1, 4096, dct, want_bits=12)[1] == 0 and run_open(emu, one, 1, 4096, dct, want_bits=13)[1] == E.EINVAL
    # the record is checked against the dictionary's own window: D = 1023 is the most a 2^10 frame admits
    d10 = dct[:1023]
    w10 = K.frame(d10, data[:4097], 10, 12, True, False)
    assert run_open(emu, w10, 2, 4097, d10)[1] == 0
    b = bytearray(w10)
    struct.pack_into("<I", b, 32 + 16, 1024)
    assert run_open(emu, W3.reseal(b), 2, 4097, d10)[1] == E.EINVAL


def test_the_old_launchers_refuse_a_version_3_frame(emu):
    dct, data = K.dct(), K.mixed()
    for store in (False, True):
        frame = K.frame(dct, data, 15, 12, store, False)
        buf = aligned_copy(frame)
        for masked in (False, True):
            in_off, out_off = np.full(4, 99, np.uint64), np.full(4, 99, np.uint64)
            stored = np.full(4, 99, np.uint32) if masked else None
            st = np.full(1, -1, np.int32)
            assert emu.emu_frame_open_old(_p(buf), C.c_uint64(len(frame)), 3, C.c_uint64(len(data)), 0, 3, _p(in_off),
                                          _p(out_off), _p(stored), _p(st), 0) == 0
            assert int(st[0]) == E.EINVAL and not in_off.any() and not out_off.any()
            assert stored is None or not stored[:3].any()


def test_the_old_launchers_take_what_they_took(emu):
    """versions 1 and 2 through the launchers there were, with and without the caller's block_bits"""
    data = K.mixed()
    for frame in (W.write_frame(data, 15, 12), W2.write_frame(data, 15, 12)):
        buf = aligned_copy(frame)
        starts = [b["payload_off"] for b in W2.blocks(frame)] + [len(frame)]
        for want_bits, want in ((0, 0), (12, 0), (13, E.EINVAL)):
            in_off, out_off = np.full(4, 99, np.uint64), np.full(4, 99, np.uint64)
            stored, st = np.full(4, 99, np.uint32), np.full(1, -1, np.int32)
            emu.emu_frame_open_old(_p(buf), C.c_uint64(len(frame)), 3, C.c_uint64(len(data)), 0, 3, _p(in_off),
                                   _p(out_off), _p(stored), _p(st), want_bits)
            assert int(st[0]) == want
            assert in_off.tolist() == (starts if want == 0 else [0] * 4)


# ---------------------------------------------------------------------------------- the decode chain
@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_decode_chain_with_the_dictionary_under_the_mask(emu, waves):
    dct, data = K.dct(), K.mixed()
    frame = K.frame(dct, data, 15, 12, True, False)
    d = _dict(dct)
    for first, n_sel in ((0, 3), (1, 2)):
        buf = aligned_copy(frame)
        lo, hi = first * 4096, min((first + n_sel) * 4096, len(data))
        in_off, out_off = np.zeros(n_sel + 1, np.uint64), np.zeros(n_sel + 1, np.uint64)
        stored, st = np.zeros(n_sel + 1, np.uint32), np.full(1, -1, np.int32)
        out = np.full(hi - lo + GUARD, 0xA5, np.uint8)
        toks = np.full(hi - lo + 64, 0xDEADBEEF, np.uint32)
        cnt, err = np.full(n_sel, 0xDEADBEEF, np.uint32), np.full(n_sel, -1, np.int32)
        rc = emu.emu_frame_decode_v3(_p(buf), C.c_uint64(len(frame)), 3, C.c_uint64(len(data)), first, n_sel, _p(d),
                                     len(dct), _p(in_off), _p(out_off), _p(stored), _p(st), _p(out), _p(toks), _p(cnt),
                                     _p(err), waves)
        assert rc == 0 and int(st[0]) == 0 and not err.any()
        assert out[:hi - lo].tobytes() == data[lo:hi] and (out[hi - lo:] == 0xA5).all()
        assert stored[:n_sel].tolist() == [0, 1, 0][first:first + n_sel]
    # a wrong dictionary: nothing is decoded, nothing is written
    buf, wrong = aligned_copy(frame), _dict(dct[:-1])
    out = np.full(len(data) + GUARD, 0xA5, np.uint8)
    in_off, out_off, stored = np.zeros(4, np.uint64), np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    toks, cnt, err = np.zeros(len(data) + 64, np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.int32)
    st = np.full(1, -1, np.int32)
    emu.emu_frame_decode_v3(_p(buf), C.c_uint64(len(frame)), 3, C.c_uint64(len(data)), 0, 3, _p(wrong), len(dct) - 1,
                            _p(in_off), _p(out_off), _p(stored), _p(st), _p(out), _p(toks), _p(cnt), _p(err), waves)
    assert int(st[0]) == E.EILSEQ and (out == 0xA5).all()


# ---------------------------------------------------------------------------------- the ranged read
def _ranges(data):
    return K.RANGES + ((0, len(data)), (len(data) - 1, 1), (4096, 4096), (0, 1))


def run_plan(em, data, at, n, err, status=0, extra_err=()):
    """the read plan and the copy over the covering blocks as they would lie decoded in the scratch"""
    first, end = at >> 12, ((at + n - 1) >> 12) + 1
    blocks = np.frombuffer(data[first * 4096:min(end * 4096, len(data))], np.uint8).copy()
    out = np.full(n + 2 * GUARD, 0xA5, np.uint8)
    errs = np.asarray(list(err) + list(extra_err) + [0], np.int32)
    plan, st = np.full(6, 0x7777, np.uint64), np.full(1, status, np.int32)
    em.emu_frame_read_plan(_p(errs), end - first, C.c_uint64(at - first * 4096), C.c_uint64(n), _p(blocks),
                           _p(out[GUARD:]), _p(plan), _p(st))
    assert plan[5] == 0x7777 and plan[:4].tolist() == [at - first * 4096, 0x7777, 0, n]
    return int(st[0]), out, end - first


def test_read_plan_and_copy(emu):
    data = K.mixed()
    for at, n in _ranges(data):
        covering = ((at + n - 1) >> 12) - (at >> 12) + 1
        st, out, n_sel = run_plan(emu, data, at, n, [0] * covering)
        assert st == 0 and n_sel == covering
        assert out[GUARD:GUARD + n].tobytes() == data[at:at + n], (at, n)
        assert (out[:GUARD] == 0xA5).all() and (out[GUARD + n:] == 0xA5).all(), (at, n)
        # an errno behind the covering blocks' entries is not this read's
        st, out, _ = run_plan(emu, data, at, n, [0] * covering, extra_err=[E.EILSEQ])
        assert st == 0 and out[GUARD:GUARD + n].tobytes() == data[at:at + n]
        for k in range(covering):                            # any covering block's errno: nothing is delivered
            err = [0] * covering
            err[k] = E.EILSEQ
            if k + 1 < covering:
                err[k + 1] = E.EINVAL                        # the first one is the status
            st, out, _ = run_plan(emu, data, at, n, err)
            assert st == E.EILSEQ and (out == 0xA5).all(), (at, n, k)
        # the frame's status comes before any block's
        st, out, _ = run_plan(emu, data, at, n, [E.EINVAL] * covering, status=E.E2BIG)
        assert st == E.E2BIG and (out == 0xA5).all()
    # more covering blocks than the plan kernel has lanes: the first non-zero entry, not any
    errs = [0] * 700
    errs[300], errs[44 + 256] = E.EINVAL, E.EINVAL
    errs[299], errs[613] = E.ENOBUFS, E.EILSEQ
    blocks, out = np.zeros(64, np.uint8), np.full(64, 0xA5, np.uint8)
    plan, st = np.zeros(5, np.uint64), np.zeros(1, np.int32)
    emu.emu_frame_read_plan(_p(np.asarray(errs, np.int32)), 700, C.c_uint64(3), C.c_uint64(20), _p(blocks), _p(out), _p(plan), _p(st))
    assert int(st[0]) == E.ENOBUFS and (out == 0xA5).all()


def run_read(em, frame, data, dct, at, n, block_bits=12, waves=1):
    first, end = at >> block_bits, ((at + n - 1) >> block_bits) + 1
    n_sel = end - first
    sel = min(end << block_bits, len(data)) - (first << block_bits)
    buf, d = aligned_copy(frame), _dict(dct)
    in_off, out_off = np.zeros(n_sel + 1, np.uint64), np.zeros(n_sel + 1, np.uint64)
    crc, st = np.zeros(n_sel + 1, np.uint32), np.full(1, -1, np.int32)
    blocks, out = np.full(sel + GUARD, 0xA5, np.uint8), np.full(n + 2 * GUARD, 0xA5, np.uint8)
    toks, cnt, err = np.zeros(sel + 64, np.uint32), np.zeros(n_sel, np.uint32), np.full(n_sel, -1, np.int32)
    plan = np.zeros(5, np.uint64)
    n_blocks = (len(data) + (1 << block_bits) - 1) >> block_bits
    rc = em.emu_frame_read_v3(_p(buf), C.c_uint64(len(frame)), n_blocks, C.c_uint64(len(data)), block_bits,
                              C.c_uint64(at), C.c_uint64(n), _p(d), len(dct), _p(in_off), _p(out_off), _p(crc), _p(st),
                              _p(blocks), _p(toks), _p(cnt), _p(err), _p(plan), _p(out[GUARD:]), waves)
    assert rc == 0 and (blocks[sel:] == 0xA5).all()
    return int(st[0]), err.tolist(), out


@pytest.mark.parametrize("store", [False, True])
def test_ranged_read_through_the_whole_chain(emu, store):
    dct, data = K.dct(), K.mixed()
    frame = K.frame(dct, data, 15, 12, store, False)
    # (without SQZ_FRAME_STORED the block of noise is a stream, which the emulator takes seconds to decode: two ranges)
    for at, n in _ranges(data) if store else ((4090, 12), (8500, 596)):
        st, err, out = run_read(emu, frame, data, dct, at, n)
        assert st == 0 and not any(err), (at, n)
        assert out[GUARD:GUARD + n].tobytes() == data[at:at + n], (at, n)
        assert (out[:GUARD] == 0xA5).all() and (out[GUARD + n:] == 0xA5).all(), (at, n)
    # damage in block 2: a read that it covers delivers nothing, one that it does not is not troubled
    bad = bytearray(frame)
    bad[W3.blocks(frame)[2]["payload_off"] + 9] ^= 0x40
    st, err, out = run_read(emu, bytes(bad), data, dct, 8000, 400)
    assert st != 0 and err[0] == 0 and err[1] == st and (out == 0xA5).all()
    st, err, out = run_read(emu, bytes(bad), data, dct, 4090, 12)
    assert st == 0 and err == [0, 0] and out[GUARD:GUARD + 12].tobytes() == data[4090:4102]
    # damage in the content of a stored block, which no decoder looks at: the checksum notices
    if store:
        bad = bytearray(frame)
        bad[W3.blocks(frame)[1]["payload_off"] + 100] ^= 1
        st, err, out = run_read(emu, bytes(bad), data, dct, 4090, 12)
        assert st == E.EILSEQ and err == [0, E.EILSEQ] and (out == 0xA5).all()
    # a wrong dictionary, and a caller whose block_bits is not the frame's: the frame's status, nothing delivered
    st, err, out = run_read(emu, frame, data, dct[:-1], 100, 50)
    assert st == E.EILSEQ and err == [E.EILSEQ] and (out == 0xA5).all()
    st, err, out = run_read(emu, frame, data, dct, 100, 50, block_bits=13)
    assert st == E.EINVAL and err == [E.EINVAL] and (out == 0xA5).all()
