"""CPU: more content behind a resident frame in one call -- the plan, verdict and append-index kernels
(sqz_amd/csrc/frame.hip) by themselves, then the whole chain with the open for a list, the decode kernels, the range
copy, the checksums, the seal and the splice -- compiled by g++ against tests/emu/hip/hip_runtime.h, run lane by lane
on the CPU wave emulator and held against the independent writers' frame of old + data (tests/frame_append_cases.py).
The encode kernels do not run here: the new blocks' streams come from the oracle as the slabs' contents.  This pins the
kernels' LOGIC without a GPU; the -m gpu tests (test_frame_append_gpu.py) pin the gfx950 build."""
import ctypes as C
import errno
import os
import subprocess
import zlib

import numpy as np
import pytest

import frame_append_cases as A
import frame_gather_cases as G
import frame_update_cases as U
import frame_writer as W
from test_frame_emu import aligned_copy
from test_frame_gather_emu import Arr, _dict, _p, u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
E = errno
BB, BITS, WB = G.BB, G.BITS, G.WB
SLAB = 2 * BB + 1024                         # sqz_bound(4096)
OLD_SEL, SLAB_SEL, STAGE_SEL = 0, 1 << 62, 2 << 62
OFF_MASK = (1 << 62) - 1


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU, "libsqz_emu_frame_append.so")
    deps = [os.path.join(EMU, f) for f in ("emu_runtime.cpp", "emu_frame_append.cpp", "hip/hip_runtime.h")] + \
           [os.path.join(CSRC, f) for f in ("frame.hip", "decode.hip", "sqz_tree.h", "sqz_device.h", "sqz_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-I" + EMU,
                               "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                               "-Wno-attributes", os.path.join(EMU, "emu_runtime.cpp"),
                               os.path.join(EMU, "emu_frame_append.cpp"), "-o", out])
    return C.CDLL(out)


def test_the_shared_inputs_are_what_they_are_there_for():
    A.check_layout()


def pad16(v):
    return (v + 15) & ~15


# ---------------------------------------------------------------------------------- the plan kernel
def run_plan(em, n, content_bytes, data_bytes, frame_win=WB, win_bits=WB):
    words = (n + 31) // 32
    bitmap, wpre, sel, ctl = Arr(words, np.uint32), Arr(words + 1, np.uint32), Arr(1, np.uint32), Arr(2, np.uint32)
    head = np.zeros(32, np.uint8)
    head[5] = frame_win
    em.emu_append_plan(_p(head), n, u64(content_bytes), u64(data_bytes), BITS, win_bits, _p(bitmap.a), _p(wpre.a),
                       _p(sel.a), _p(ctl.a))
    assert all(a.guard_ok() for a in (bitmap, wpre, sel, ctl))
    return bitmap.a.tolist(), wpre.a.tolist(), sel, ctl.a.tolist()


def test_plan_kernel_marks_the_last_block_iff_it_is_touched(emu):
    # word edges, one word, more words than one workgroup has lanes (8193 blocks: 257 words), no block at all
    for n in (0, 1, 2, 31, 32, 33, 64, 65, 300, 8192, 8193):
        words = (n + 31) // 32
        for t in (0, 1, 904, BB - 1):
            if n == 0 and t != 0:
                continue
            content_bytes = n * BB if t == 0 else (n - 1) * BB + t
            for data_bytes in (0, 1, 5 * BB):
                touched = t > 0 and data_bytes > 0
                bitmap, wpre, sel, ctl = run_plan(emu, n, content_bytes, data_bytes)
                want = [0] * words
                if touched:
                    want[(n - 1) >> 5] = 1 << ((n - 1) & 31)
                what = (n, t, data_bytes)
                assert bitmap == want and wpre == [0] * words + [1 if touched else 0], what
                assert ctl == [1 if touched else 0, 0], what
                assert sel.a.tolist() == [n - 1] if touched else sel.untouched(), what
    # the verdict on the request: a frame of another window
    for frame_win, win_bits, want in ((WB, WB, 0), (WB - 1, WB, E.EINVAL), (WB, WB - 1, E.EINVAL), (10, 10, 0)):
        assert run_plan(emu, 4, 3 * BB + 904, 7, frame_win, win_bits)[3] == [1, want]
        assert run_plan(emu, 4, 4 * BB, 7, frame_win, win_bits)[3] == [0, want]


# ---------------------------------------------------------------------------------- the verdict kernel
def run_verdict(em, n, content_bytes, data_bytes, m, touched, err0=0, crc_ok=True, status=0):
    rng = np.random.default_rng(n + 1)
    frame = aligned_copy(rng.integers(0, 256, 32 + 8 * max(n, 1), dtype=np.uint8).tobytes())
    index = frame[32:].view(np.uint32)
    ctl = np.asarray([1 if touched else 0, 0], np.uint32)
    err = np.asarray([err0, E.EIO, 0], np.int32)          # entry 1 is the pseudo-block's: nobody's
    crc = np.asarray([(int(index[2 * (n - 1) + 1]) if n else 0) ^ (0 if crc_ok else 1), 0x77777777, 0], np.uint32)
    st, enc = np.asarray([status], np.int32), np.full(1, 0xDEAD, np.uint32)
    copy, in_off, slab_off = Arr(5, np.uint64), Arr(m + 1, np.uint64), Arr(m + 1, np.uint64)
    em.emu_append_verdict(_p(frame), n, _p(ctl), _p(err), _p(crc), BITS, u64(content_bytes), u64(data_bytes), m, u64(SLAB),
                          _p(st), _p(enc), _p(copy.a), _p(in_off.a), _p(slab_off.a))
    assert copy.guard_ok() and in_off.guard_ok() and slab_off.guard_ok()
    assert slab_off.a.tolist() == [k * SLAB for k in range(m + 1)]
    c = copy.a.tolist()
    return int(st[0]), int(enc[0]), c[:4] + [c[4] & 0xFFFFFFFF], in_off.a.tolist()


def test_verdict_kernel_orders_the_statuses_and_lays_the_encoders_blocks_out(emu):
    n = 300
    # (t, data bytes): the data ends in the touched block, on its edge, behind it; 600 blocks: three turns per lane
    for t, data_bytes in ((904, 1), (904, 3192), (904, 3193), (0, 1), (0, BB), (0, 2 * BB + 5), (100, 600 * BB - 100),
                          (904, 0), (0, 0)):
        content_bytes = n * BB if t == 0 else (n - 1) * BB + t
        touched = t > 0 and data_bytes > 0
        head = t if touched else 0
        end = head + data_bytes
        m = (end + BB - 1) // BB if data_bytes else 0
        what = (t, data_bytes)
        st, enc, copy, in_off = run_verdict(emu, n, content_bytes, data_bytes, m, touched)
        assert (st, enc) == (0, m), what
        assert copy == [0, head if data_bytes else 0, 0, data_bytes, 1 if data_bytes else 0], what
        assert in_off == [min(k * BB, end) for k in range(m + 1)], what
        off = [0] * (m + 1)
        if touched:
            # the decoder's errno in front of the checksum; either switches the copy and the encoder off
            for err0, crc_ok, want in ((E.EBADMSG, True, E.EBADMSG), (E.EIO, False, E.EIO), (0, False, E.EILSEQ)):
                st, enc, copy, in_off = run_verdict(emu, n, content_bytes, data_bytes, m, True, err0, crc_ok)
                assert (st, enc, copy[4], in_off) == (want, m, 0, off), what
        else:
            # nothing was decoded: whatever the entries hold is nobody's
            st, enc, copy, in_off = run_verdict(emu, n, content_bytes, data_bytes, m, False, E.EIO, False)
            assert (st, enc) == (0, m) and copy[4] == (1 if data_bytes else 0), what
        # a status of the open kernel's stays, whatever the slot holds, and counts no block
        st, enc, copy, in_off = run_verdict(emu, n, content_bytes, data_bytes, m, touched, E.EIO, False, status=E.EILSEQ)
        assert (st, enc, copy[4], in_off) == (E.EILSEQ, 0, 0, off), what
    # an empty frame
    st, enc, copy, in_off = run_verdict(emu, 0, 0, BB + 1, 2, False)
    assert (st, enc, copy, in_off) == (0, 2, [0, 0, 0, BB + 1, 1], [0, BB, BB + 1])


# ---------------------------------------------------------------------------------- the append-index kernel
def new_blocks_of(name, data):
    """(keep, m, n', the m blocks of tail || data, the staging area's bytes)"""
    old = A.old_content(name)
    t, touched, keep, m, n_new = A.shape(name, len(data))
    stage = (old[len(old) - t:] if touched else b"") + data
    blocks = W.blocks_of(stage, BITS)
    assert len(blocks) == m and blocks == W.blocks_of(old + data, BITS)[keep:]
    return keep, m, n_new, blocks, stage


def encoder_results(blocks, version, m, enc_err=None):
    streams = [U.stream_of(b, 1 if version == 2 else version, False) for b in blocks]
    out_bytes = np.asarray([len(s) for s in streams] + [0], np.uint64)
    err = np.asarray([(enc_err or {}).get(k, 0) for k in range(m)] + [0], np.int32)
    slabs = aligned_copy(bytes(max(m, 1) * SLAB))
    for k, s in enumerate(streams):
        slabs[k * SLAB:k * SLAB + len(s)] = np.frombuffer(s, np.uint8)
    return out_bytes, err, slabs


def run_index(em, name, version, data, capacity=None, enc_err=None, status=0):
    """the kernel, then the splice over its table: the whole new frame but for index_crc"""
    old_content, old = A.old_content(name), A.old_frame(name, version)
    n = (len(old_content) + BB - 1) // BB
    keep, m, n_new, blocks, stage = new_blocks_of(name, data)
    out_bytes, err, slabs = encoder_results(blocks, version, m, enc_err)
    crc_new = np.asarray([zlib.crc32(b) for b in blocks] + [0], np.uint32)
    staging = aligned_copy(stage + bytes([0x5A]) * 16)
    want = A.frame_of(old_content + data, version)
    capacity = len(want) if capacity is None else capacity
    frame = Arr(capacity, np.uint8, align=True)
    seg_dst, seg_src, seg_len = Arr(m + 2, np.uint64), Arr(m + 1, np.uint64), Arr(m + 1, np.uint64)
    idx_off, fb, st = Arr(2, np.uint64), Arr(1, np.uint64), np.asarray([status], np.int32)
    buf = aligned_copy(old)
    em.emu_append_index(_p(buf), n, u64(len(old_content)), u64(len(data)), m, 1 if version == 3 else 0, _p(out_bytes),
                        _p(err), _p(crc_new), u64(SLAB), _p(frame.a), u64(capacity), _p(seg_dst.a), _p(seg_src.a),
                        _p(seg_len.a), _p(idx_off.a), _p(fb.a), _p(st))
    assert all(a.guard_ok() for a in (frame, seg_dst, seg_src, seg_len, idx_off, fb))
    em.emu_append_splice(_p(buf), _p(slabs), _p(staging), _p(frame.a), _p(seg_dst.a), _p(seg_src.a), _p(seg_len.a),
                         m + 1, u64(capacity))
    assert frame.guard_ok()
    return {"status": int(st[0]), "frame_bytes": int(fb.a[0]), "frame": frame, "want": want, "idx_off": idx_off.a.tolist(),
            "seg_dst": seg_dst.a.tolist(), "seg_src": seg_src.a.tolist(), "seg_len": seg_len.a.tolist(), "n_new": n_new,
            "keep": keep, "m": m}


def _same_but_for_the_seal(frame, want):
    got = bytearray(frame.a.tobytes())
    return bytes(got[:28]) + bytes(got[32:]) == want[:28] + want[32:] and got[28:32] == bytes(4)


@pytest.mark.parametrize("version", [1, 2, 3])
def test_append_index_kernel_and_the_table_it_leaves(emu, version):
    record = 8 if version == 3 else 0
    for name, length in A.cases():
        data = A.data_of(name, length)
        what = (version, name, length)
        got = run_index(emu, name, version, data)
        want, n_new, keep, m = got["want"], got["n_new"], got["keep"], got["m"]
        assert (got["status"], got["frame_bytes"]) == (0, len(want)), what
        assert _same_but_for_the_seal(got["frame"], want), what
        assert got["idx_off"] == [32, 32 + 8 * n_new + record], what
        # segment 0 is the kept run, moved from the old payload_off to the new one; the touched block's stream stays behind
        old = A.old_frame(name, version)
        n = (len(A.old_content(name)) + BB - 1) // BB
        kept = sum(e["payload_bytes"] for e in G.block_entries(old, version)[:keep])
        seg_dst = got["seg_dst"]
        assert seg_dst == sorted(seg_dst) and seg_dst[0] == pad16(32 + 8 * n_new + record) and seg_dst[-1] == len(want), what
        assert got["seg_src"][0] == OLD_SEL | pad16(32 + 8 * n + record) and got["seg_len"][0] == kept, what
        assert seg_dst[1] - seg_dst[0] == kept, what
        for k, e in enumerate(G.block_entries(want, version)[keep:]):
            src = got["seg_src"][k + 1]
            assert src == (STAGE_SEL | k * BB if e["stored"] else SLAB_SEL | k * SLAB), what
            assert got["seg_len"][k + 1] == (e["content_bytes"] if e["stored"] else e["payload_bytes"]), what
        if length in (0, 1, A.fill(name) + 1):
            # one byte short: E2BIG, the size it takes, and not one byte of the frame
            got = run_index(emu, name, version, data, capacity=len(want) - 1)
            assert (got["status"], got["frame_bytes"], got["idx_off"]) == (E.E2BIG, len(want), [0, 0]), what
            assert got["frame"].untouched() and not any(got["seg_dst"]), what
            # a status from before: kept, and nothing is done
            got = run_index(emu, name, version, data, status=E.EILSEQ)
            assert (got["status"], got["frame_bytes"], got["idx_off"]) == (E.EILSEQ, 0, [0, 0]), what
            assert got["frame"].untouched() and not any(got["seg_dst"]), what
        if m >= 1 and length in (1, A.fill(name) + BB + 904):
            # an encoder errno: the first in ascending order, in front of the capacity, no size, nothing written
            bad = {m - 1: E.ENOBUFS}
            if m > 1:
                bad[0] = E.EINVAL
            got = run_index(emu, name, version, data, enc_err=bad, capacity=64)
            assert (got["status"], got["frame_bytes"]) == (bad.get(0, E.ENOBUFS), 0) and got["frame"].untouched(), what


def test_append_index_kernel_refuses_a_size_no_entry_holds(emu):
    name, data = "whole", A.data_of("whole", 5000)
    keep, m, n_new, blocks, stage = new_blocks_of(name, data)
    for version, size, want in ((1, 12, E.EINVAL), (2, 1 << 35, E.EINVAL), (3, 1 << 34, E.EINVAL), (1, 1 << 34, E.E2BIG)):
        old_content, old = A.old_content(name), A.old_frame(name, version)
        out_bytes = np.asarray([8, size, 0], np.uint64)
        err, crc_new = np.zeros(3, np.int32), np.zeros(3, np.uint32)
        frame = Arr(1 << 16, np.uint8, align=True)
        seg_dst, seg_src, seg_len = Arr(m + 2, np.uint64), Arr(m + 1, np.uint64), Arr(m + 1, np.uint64)
        idx_off, fb, st = Arr(2, np.uint64), Arr(1, np.uint64), np.asarray([0], np.int32)
        emu.emu_append_index(_p(aligned_copy(old)), 4, u64(len(old_content)), u64(len(data)), m, 1 if version == 3 else 0,
                             _p(out_bytes), _p(err), _p(crc_new), u64(SLAB), _p(frame.a), u64(1 << 16), _p(seg_dst.a),
                             _p(seg_src.a), _p(seg_len.a), _p(idx_off.a), _p(fb.a), _p(st))
        assert int(st[0]) == want and frame.untouched() and not any(seg_dst.a.tolist()), (version, size)
        assert all(a.guard_ok() for a in (seg_dst, seg_src, seg_len, idx_off, fb))


# ---------------------------------------------------------------------------------- the whole chain
def run_append(em, name, version, length, frame=None, data=None, dct=None, capacity=None, win_bits=WB, enc_err=None,
               avail=None):
    old_content = A.old_content(name)
    frame = A.old_frame(name, version) if frame is None else frame
    data = A.data_of(name, length) if data is None else data
    n = (len(old_content) + BB - 1) // BB
    words = (n + 31) // 32
    keep, m, n_new, blocks, stage = new_blocks_of(name, data)
    touched = keep < n
    want = A.frame_of(old_content + data, version)
    capacity = len(want) if capacity is None else capacity
    arrays = [Arr(words, np.uint32), Arr(words + 1, np.uint32), Arr(2, np.uint32), Arr(1, np.uint32), Arr(3, np.uint64),
              Arr(3, np.uint64), Arr(2, np.uint32), Arr(2, np.uint32), Arr(2, np.uint32), Arr(2, np.int32),
              Arr(BB + 64, np.uint32), Arr(2, np.uint32), Arr(len(stage) + 16, np.uint8, align=True), Arr(5, np.uint64),
              Arr(m + 1, np.uint64), Arr(m + 1, np.uint64), Arr(m, np.uint64), Arr(m, np.int32), Arr(m, np.uint32),
              Arr(m + 2, np.uint64), Arr(m + 1, np.uint64), Arr(m + 1, np.uint64), Arr(m * SLAB, np.uint8, align=True)]
    # what the encoder would leave: the oracle's streams of the new blocks
    out_bytes, errs, slabs = arrays[16], arrays[17], arrays[22]
    guards = [a for k, a in enumerate(arrays) if k not in (16, 17, 22)]
    for k, b in enumerate(blocks):
        s = U.stream_of(b, 1 if version == 2 else version, False)
        out_bytes.a[k] = len(s)
        errs.a[k] = (enc_err or {}).get(k, 0)
        slabs.a[k * SLAB:k * SLAB + len(s)] = np.frombuffer(s, np.uint8)
    ptrs = (C.c_void_p * len(arrays))(*[a.a.ctypes.data for a in arrays])
    new = Arr(capacity, np.uint8, align=True)
    fb, enc, st = Arr(1, np.uint64), np.full(1, 0xDEAD, np.uint32), np.full(1, -1, np.int32)
    if version == 3 and dct is None:
        dct = G.dct()
    d = _dict(dct) if dct is not None else None
    buf, dbuf = aligned_copy(frame), aligned_copy(data + bytes(16))
    rc = em.emu_frame_append(_p(buf), u64(len(frame) if avail is None else avail), n, u64(len(old_content)), win_bits, BITS,
                             _p(dbuf), u64(len(data)), _p(d), len(dct) if dct is not None else 0, _p(new.a), u64(capacity),
                             _p(fb.a), _p(enc), _p(st), ptrs, u64(SLAB), m, n_new, 1 if touched else 0)
    assert rc == 0
    assert all(a.guard_ok() for a in guards) and new.guard_ok() and fb.guard_ok()
    return {"status": int(st[0]), "encoded": int(enc[0]), "new": new, "frame_bytes": int(fb.a[0]), "want": want, "m": m,
            "staging": arrays[12], "stage": stage, "err": arrays[9], "keep": keep}


def check_frame(got, what=None):
    assert (got["status"], got["frame_bytes"], got["encoded"]) == (0, len(got["want"]), got["m"]), what
    assert got["new"].a.tobytes() == got["want"], what
    assert got["staging"].a[:len(got["stage"])].tobytes() == got["stage"], what


def refused(got, status, encoded=None, frame_bytes=0):
    assert (got["status"], got["frame_bytes"]) == (status, frame_bytes), (got["status"], got["frame_bytes"])
    assert encoded is None or got["encoded"] == encoded
    assert got["new"].untouched()
    return True


CHAIN = [(v, name) for name in A.OLD for v in (1, 2, 3)]


@pytest.mark.parametrize("version,name", CHAIN, ids=[f"v{v}-{n}" for v, n in CHAIN])
def test_append_through_the_whole_chain(emu, version, name):
    for length in A.lengths(name):
        got = run_append(emu, name, version, length)
        check_frame(got, (version, name, length))
        if length == 0:                                  # no data: the old frame's exact bytes
            assert got["new"].a.tobytes() == A.old_frame(name, version)


@pytest.mark.parametrize("version", [1, 2, 3])
def test_a_long_append_gives_lanes_two_entries_and_none(emu, version):
    name, length = A.cases()[-1]
    assert A.shape(name, length)[4] == 260
    check_frame(run_append(emu, name, version, length), (version, name, length))


def test_every_refusal_in_the_calls_order_writes_nothing(emu):
    name = "short"                                       # a N b t: the last block is touched
    length = A.fill(name) + BB + 904                     # three new blocks
    m = A.shape(name, length)[3]
    assert m == 3
    for version in (1, 2, 3):
        frame = A.old_frame(name, version)
        entries = G.block_entries(frame, version)
        # 1. the frame's own status in front of everything else: the dictionary, the index checksum, the other window
        wrong = dict(dct=G.dct()[:-1]) if version == 3 else dict(dct=G.dct())
        got = run_append(emu, name, version, length, enc_err={0: E.ENOBUFS}, capacity=64, **wrong)
        assert refused(got, E.EILSEQ if version == 3 else E.EINVAL, 0) and got["staging"].untouched()
        bad = bytearray(frame)
        bad[32 + 3] ^= 0x10
        got = run_append(emu, name, version, length, frame=bytes(bad), win_bits=14, capacity=64)
        assert refused(got, E.EILSEQ, 0) and got["staging"].untouched()
        got = run_append(emu, name, version, length, win_bits=14, enc_err={0: E.ENOBUFS}, capacity=64)
        assert refused(got, E.EINVAL, 0) and got["staging"].untouched()
        #    no data: the frame's status, not a copy
        assert refused(run_append(emu, name, version, 0, win_bits=14), E.EINVAL, 0)
        # 2. a damaged touched block, in front of an encoder's errno and a capacity that would not do: the decoder's
        #    errno where it has one, else EILSEQ
        last = entries[-1]
        for at in (3, 9, last["payload_bytes"] - 12):
            bad = bytearray(frame)
            bad[last["payload_off"] + at] ^= 0x40
            got = run_append(emu, name, version, length, frame=bytes(bad), enc_err={0: E.ENOBUFS}, capacity=64)
            slot_err = int(got["err"].a[0])
            assert refused(got, slot_err if slot_err != 0 else E.EILSEQ, m), (version, at, slot_err)
        #    the stream as it was and an index entry with another CRC-32 (the index's own checksum made good): the
        #    decoder succeeds, so it is EILSEQ and nothing else
        bad = bytearray(frame)
        bad[32 + 8 * 3 + 4] ^= 0x01
        index_end = 32 + 8 * 4 + (8 if version == 3 else 0)
        bad[28:32] = zlib.crc32(bytes(bad[:28]) + bytes(bad[32:index_end])).to_bytes(4, "little")
        got = run_append(emu, name, version, length, frame=bytes(bad), enc_err={0: E.ENOBUFS}, capacity=64)
        assert int(got["err"].a[0]) == 0 and refused(got, E.EILSEQ, m)
        # 3. an encoder's errno, the first in ascending order, in front of the capacity
        got = run_append(emu, name, version, length, enc_err={1: E.ENOBUFS, 2: E.EINVAL}, capacity=64)
        assert refused(got, E.ENOBUFS, m)
        # 4. E2BIG one byte short, with the size it takes
        need = len(A.expected(name, length, version))
        assert refused(run_append(emu, name, version, length, capacity=need - 1), E.E2BIG, m, need)
        check_frame(run_append(emu, name, version, length, capacity=need))
        #    and with no data: the copy does not fit either
        assert refused(run_append(emu, name, version, 0, capacity=len(frame) - 1), E.E2BIG, 0, len(frame))


def test_a_damaged_stored_touched_block_is_eilseq_and_a_damaged_kept_block_stays_as_it_is(emu):
    # noise_tail: the ragged last block is stored in versions 2 and 3
    for version in (2, 3):
        frame = A.old_frame("noise_tail", version)
        last = G.block_entries(frame, version)[-1]
        assert last["stored"] == 1
        bad = bytearray(frame)
        bad[last["payload_off"] + 9] ^= 0x40
        got = run_append(emu, "noise_tail", version, 100, frame=bytes(bad))
        assert refused(got, E.EILSEQ, 1)
        # the same damage with nothing to append, or in a frame whose last block is whole: nobody decodes it
    # a damaged kept block: status 0, and the new frame is the expected one with that stream as damaged as it was
    for version, name, victim in ((2, "short", 1), (1, "short", 1), (3, "whole", 3), (2, "short", 3)):
        frame = A.old_frame(name, version)
        entry = G.block_entries(frame, version)[victim]
        bad = bytearray(frame)
        bad[entry["payload_off"] + 9] ^= 0x40
        # a victim that is the ragged last block is kept only when there is no data
        length = 0 if victim == 3 and name == "short" else A.fill(name) + BB + 904
        got = run_append(emu, name, version, length, frame=bytes(bad))
        assert got["status"] == 0 and got["frame_bytes"] == len(got["want"]) and got["keep"] > victim
        want = bytearray(got["want"])
        want[G.block_entries(got["want"], version)[victim]["payload_off"] + 9] ^= 0x40
        assert got["new"].a.tobytes() == bytes(want), (version, name, victim)
