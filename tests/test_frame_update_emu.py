"""CPU: many ranges written into a resident frame in one call -- the plan, verdict, merge-index and splice kernels
(sqz_amd/csrc/frame.hip) by themselves, then the whole chain behind the gather's mark, select and open and the decode
kernels -- compiled by g++ against tests/emu/hip/hip_runtime.h, run lane by lane on the CPU wave emulator and held
against the independent writers' frame of the patched content (tests/frame_update_cases.py).  The encode kernels do
not run here: the touched blocks' new streams come from the oracle as the slabs' contents.  This pins the kernels'
LOGIC without a GPU; the -m gpu tests (test_frame_update_gpu.py) pin the gfx950 build."""
import ctypes as C
import errno
import os
import subprocess
import zlib

import numpy as np
import pytest

import frame_gather_cases as G
import frame_update_cases as U
import frame_writer as W
from test_frame_emu import aligned_copy
from test_frame_gather_emu import Arr, FILL, _bitmap, _dict, _p, _ranges, u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
E = errno
BB, BITS, WB = G.BB, G.BITS, G.WB
SLAB = 2 * BB + 1024                         # sqz_bound(4096)
OLD, SLAB_SEL, SLOT_SEL = 0, 1 << 62, 2 << 62
ALL = (1 << 64) - 1


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU, "libsqz_emu_frame_update.so")
    deps = [os.path.join(EMU, f) for f in ("emu_runtime.cpp", "emu_frame_update.cpp", "hip/hip_runtime.h")] + \
           [os.path.join(CSRC, f) for f in ("frame.hip", "decode.hip", "sqz_tree.h", "sqz_device.h", "sqz_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-I" + EMU,
                               "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                               "-Wno-attributes", os.path.join(EMU, "emu_runtime.cpp"),
                               os.path.join(EMU, "emu_frame_update.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.emu_update_chunk.restype = C.c_uint64
    return lib


def test_the_shared_inputs_are_what_they_are_there_for():
    U.check_layout()


def _wpre(words):
    return np.asarray([sum(bin(w).count("1") for w in words[:k]) for k in range(len(words) + 1)], np.uint32)


# ---------------------------------------------------------------------------------- the splice kernel
def run_splice(em, segs, m, base=48, most=None, tail_guard=64):
    """segs: [(selector, source offset, destination bytes, source bytes or None)]; returns what the payload must be"""
    rng = np.random.default_rng(len(segs) + m)
    src = {OLD: aligned_copy(rng.integers(0, 256, 1 << 18, dtype=np.uint8).tobytes()),
           SLAB_SEL: aligned_copy(rng.integers(0, 256, 1 << 18, dtype=np.uint8).tobytes()),
           SLOT_SEL: aligned_copy(rng.integers(0, 256, 1 << 18, dtype=np.uint8).tobytes())}
    n_seg = 2 * m + 1
    assert len(segs) <= n_seg
    seg_dst, seg_src, seg_len, want, at = [], [], [], b"", base
    for sel, off, n, have in segs:
        assert n % 8 == 0 and off % 8 == 0
        seg_dst.append(at); seg_src.append(sel | off); seg_len.append(ALL if have is None else have)
        got = src[sel][off:off + (n if have is None else min(have, n))].tobytes()
        want += got + bytes(n - len(got))
        at += n
    seg_dst += [at] * (n_seg + 1 - len(segs))
    seg_src += [0] * (n_seg - len(segs))
    seg_len += [0] * (n_seg - len(segs))
    dst = Arr(at + tail_guard, np.uint8, align=True)
    em.emu_update_splice(_p(src[OLD]), _p(src[SLAB_SEL]), _p(src[SLOT_SEL]), _p(dst.a), _p(np.asarray(seg_dst, np.uint64)),
                         _p(np.asarray(seg_src + [0], np.uint64)), _p(np.asarray(seg_len + [0], np.uint64)), m,
                         u64(at - base if most is None else most))
    assert dst.guard_ok() and (dst.a[:base] == FILL).all() and (dst.a[at:] == FILL).all()
    assert dst.a[base:at].tobytes() == want, [s[2] for s in segs]
    return at - base


def test_splice_kernel_lengths_alignments_chunk_edges_and_empty_runs(emu):
    chunk = int(emu.emu_update_chunk())
    assert chunk % 16 == 0
    lengths = [0, 8, 16, 24, chunk - 8, chunk, chunk + 8, 3 * chunk + 8]
    sels = [OLD, SLAB_SEL, OLD, SLOT_SEL]
    seen = set()
    for rot in range(len(lengths)):
        for parity in (0, 8):
            order = lengths[rot:] + lengths[:rot]
            segs, at = [], 48
            for j, n in enumerate(order):
                off = 1024 * j + 16 * (j % 3) + (parity if j % 2 == 0 else 8 - parity)
                segs.append((sels[j % 4], off, n, None))
                if n >= 16:
                    seen.add((off % 16, at % 16))
                at += n
            for most in (None, 1):                       # a workgroup per chunk, and one workgroup for all of them
                run_splice(emu, segs, 4, most=most)
    assert seen == {(0, 0), (0, 8), (8, 0), (8, 8)}
    # a chunk edge exactly on a segment edge and inside one; the payload ending in mid-row
    run_splice(emu, [(OLD, 64, chunk, None), (SLAB_SEL, 8, chunk, None), (OLD, 16, 8, None)], 1)
    run_splice(emu, [(OLD, 72, chunk - 24, None), (SLAB_SEL, 0, 48, None), (OLD, 16, chunk, None)], 1)
    # several empty kept runs in a row (adjacent touched blocks), around half rows
    segs = [(OLD, 48, 0, None), (SLAB_SEL, 0, 24, None), (OLD, 80, 0, None), (SLOT_SEL, 8, 8, None), (OLD, 80, 0, None),
            (SLAB_SEL, 4096, 40, None), (OLD, 88, 0, None), (SLOT_SEL, 8192, 4096, None), (OLD, 96, 24, None)]
    run_splice(emu, segs, 4)
    run_splice(emu, segs, 9)                             # a table wider than the count: empty segments behind
    # m = 0: the payload is one segment; and no payload at all
    assert run_splice(emu, [(OLD, 48, 3 * chunk + 40, None)], 0) == 3 * chunk + 40
    assert run_splice(emu, [(OLD, 48, 0, None)], 0) == 0
    # a stored ragged last block: its share is padded with zeros, whatever lies behind it in the slot
    for have in (1, 7, 8, 9, 15, 16, 17, 901, 904):
        run_splice(emu, [(OLD, 48, 24, None), (SLOT_SEL, 4096, (have + 7) & ~7, have), (OLD, 8, 0, None)], 1)
        run_splice(emu, [(OLD, 48, 16, None), (SLOT_SEL, 4096 + 8, (have + 7) & ~7, have), (OLD, 8, 0, None)], 1)


# ---------------------------------------------------------------------------------- the plan and verdict kernels
def run_plan(em, offsets, lengths, cap, content_bytes, touched, n, select_verdict=0, frame_win=WB, win_bits=WB):
    """update_plan_kernel + update_caps_kernel over a bitmap of the `touched` blocks"""
    R = len(offsets)
    o, ln = _ranges(offsets, lengths)
    words = _bitmap(touched, n)
    bm, wpre = np.asarray(words + [0], np.uint32), _wpre(words)
    data_off, at = [], 0
    for a, c in zip(offsets, lengths):
        data_off.append(at)
        at += c if G.valid(a, c, cap, content_bytes) else 0
    data_off = np.asarray(data_off + [at], np.uint64)
    rerr, src, dst, mask = Arr(R, np.int32), Arr(R, np.uint64), Arr(R, np.uint64), Arr(R, np.uint32)
    flags, ctl = Arr(1, np.uint32), Arr(3, np.uint32)
    ctl.a[:] = [len(touched), select_verdict, 0xDEAD]
    head = np.zeros(32, np.uint8)
    head[5] = frame_win
    em.emu_update_plan(_p(o), _p(ln), R, u64(cap), u64(content_bytes), BITS, n, _p(bm), _p(wpre), _p(data_off),
                       _p(rerr.a), _p(src.a), _p(dst.a), _p(mask.a), _p(head), win_bits, _p(flags.a), _p(ctl.a))
    assert all(a.guard_ok() for a in (rerr, src, dst, mask, flags, ctl))
    return rerr.a.tolist(), src.a.tolist(), dst.a.tolist(), mask.a.tolist(), int(flags.a[0]), ctl.a.tolist(), data_off.tolist()


def test_plan_kernel_places_every_range_and_caps_kernel_orders_the_verdicts(emu):
    n = 300
    content_bytes = (n - 1) * BB + 901
    # ranges that start in blocks of bitmap words 0, 1, 2, 3 and 9, some across a word's edge, one empty, one to the end;
    # 300 of them, so that the kernel runs in more than one workgroup
    starts = [(0, 5, 10), (31, 4000, 200), (32, 0, 4096), (33, 17, 1), (63, 4095, 2), (64, 1, 0), (100, 123, 9000),
              (299, 1, 900), (298, 4090, 6 + 901)]
    offsets = [b * BB + within for b, within, _ in starts]
    lengths = [c for _, _, c in starts]
    offsets += [(7 * k) % n * BB + k for k in range(300 - len(starts))]
    lengths += [1 + k % 50 for k in range(300 - len(starts))]
    cap = 9000
    touched = sorted({b for a, c in zip(offsets, lengths) if c for b in range(a >> BITS, ((a + c - 1) >> BITS) + 1)})
    assert any(t >= 32 for t in touched) and len(touched) < n
    slot = {b: k for k, b in enumerate(touched)}
    rerr, src, dst, mask, flag, ctl, data_off = run_plan(emu, offsets, lengths, cap, content_bytes, touched, n)
    assert not any(rerr) and flag == 0 and ctl == [len(touched), 0, 0]
    assert src == data_off[:-1] and mask == [1 if c else 0 for c in lengths]
    for r, (a, c) in enumerate(zip(offsets, lengths)):
        if c:
            assert dst[r] == (slot[a >> BITS] << BITS) + a % BB, r
    # invalid ranges among them: EINVAL, masked, length 0 in the data's layout, and the flag
    bad_o = offsets[:5] + [content_bytes + 1, content_bytes - 3, 0, 1 << 63] + offsets[5:]
    bad_l = lengths[:5] + [0, 4, cap + 1, 1 << 63] + lengths[5:]
    rerr, src, dst, mask, flag, ctl, data_off = run_plan(emu, bad_o, bad_l, cap, content_bytes, touched, n)
    assert rerr == [0] * 5 + [E.EINVAL] * 4 + [0] * (len(offsets) - 5) and flag == 1 and ctl[1:] == [E.ERANGE, 0]
    assert mask[5:9] == [0] * 4 and dst[9:] == [((slot[a >> BITS] << BITS) + a % BB) if c else 0
                                                for a, c in zip(offsets[5:], lengths[5:])]
    assert src[9:] == data_off[9:-1]
    # the verdict word, in the call's order: another window, an invalid range, the cap on the blocks, the data's size
    few_o, few_l = [10, 5000], [20, 30]
    for select_verdict, invalid, frame_win, want in (
            (0, False, WB, [0, 0]), (E.ENOBUFS, False, WB, [E.ENOBUFS, 0]), (E.ENOSPC, False, WB, [E.ENODATA, 0]),
            (E.ENOBUFS, True, WB, [E.ERANGE, 0]), (E.ENOSPC, True, WB, [E.ERANGE, 0]), (0, True, WB, [E.ERANGE, 0]),
            (0, False, WB - 1, [E.EINVAL, 1]), (E.ENOBUFS, True, WB + 1, [E.EINVAL, 1])):
        oo = few_o + ([content_bytes + 1] if invalid else [])
        ll = few_l + ([1] if invalid else [])
        got = run_plan(emu, oo, ll, 100, content_bytes, [0, 1], n, select_verdict=select_verdict, frame_win=frame_win)
        assert got[5] == [2] + want, (select_verdict, invalid, frame_win)
    # no range at all: only the caps kernel runs
    assert list(run_plan(emu, [], [], 0, content_bytes, [], n, select_verdict=0)[4:6]) == [0, [0, 0, 0]]


def run_verdict(em, n, content_bytes, sel, m, err_at=None, crc_at=(), status=0, refused_frame=0, n_ranges=300):
    """update_verdict_kernel over `sel` decoded slots: err_at {slot: errno}, crc_at slots whose bytes are not the entry's"""
    rng = np.random.default_rng(n)
    frame = aligned_copy(rng.integers(0, 256, 32 + 8 * n, dtype=np.uint8).tobytes())
    index = frame[32:].view(np.uint32)
    count = len(sel)
    err, crc = np.zeros(2 * m + 1, np.int32), np.full(2 * m + 1, 0x77777777, np.uint32)
    for k, b in enumerate(sel):
        crc[2 * k] = index[2 * b + 1] ^ (1 if k in crc_at else 0)
        err[2 * k] = (err_at or {}).get(k, 0)
        err[2 * k + 1] = E.EIO                             # the pseudo-block's entries are nobody's
    sel_a = np.asarray(list(sel) + [0], np.uint32)
    ctl = np.asarray([count, 0, refused_frame], np.uint32)
    st, enc = np.asarray([status], np.int32), np.asarray([count], np.uint32)
    mask, in_off, slab_off = Arr(n_ranges, np.uint32), Arr(m + 1, np.uint64), Arr(m + 1, np.uint64)
    mask.a[:] = 1
    em.emu_update_verdict(_p(frame), _p(sel_a), _p(ctl), m, _p(err), _p(crc), BITS, u64(content_bytes), u64(SLAB), n_ranges,
                          _p(st), _p(enc), _p(mask.a), _p(in_off.a), _p(slab_off.a))
    assert mask.guard_ok() and in_off.guard_ok() and slab_off.guard_ok()
    assert slab_off.a.tolist() == [k * SLAB for k in range(m + 1)]
    return int(st[0]), int(enc[0]), mask.a.tolist(), in_off.a.tolist()


def test_verdict_kernel_finds_the_first_failed_slot_and_switches_everything_behind_it_off(emu):
    n = 600
    content_bytes = (n - 1) * BB + 100
    every = list(range(n))                               # 600 slots: a thread of the 256 looks at up to three
    for sel, m in ((every, n), (every[:1], 1), (every[:257], 300), ([5, 599], 2), ([5, 7], 4), ([], 3)):
        count = len(sel)
        end = (count - 1) * BB + min(BB, content_bytes - sel[-1] * BB) if sel else 0
        st, enc, mask, in_off = run_verdict(emu, n, content_bytes, sel, m)
        assert (st, enc) == (0, count) and all(mask)
        assert in_off == [k * BB if k < count else end for k in range(m + 1)], (count, m)
    off = [0] * (n + 1)
    # the first in ascending order, whichever thread and turn finds it: slot 270 is thread 14's second, 520 thread 8's third
    for err_at, crc_at, want in (({520: E.EIO}, (), E.EIO), ({520: E.EIO, 270: E.EBADMSG}, (), E.EBADMSG),
                                 ({520: E.EIO}, (270,), E.EILSEQ), ({270: E.EBADMSG}, (260, 599), E.EILSEQ),
                                 ({8: E.ERANGE}, (8, 264), E.ERANGE), ({}, (599,), E.EILSEQ), ({0: E.EIO}, (), E.EIO),
                                 ({255: E.EIO, 256: E.EBADMSG}, (), E.EIO), ({511: E.EIO, 256: E.EBADMSG}, (), E.EBADMSG)):
        st, enc, mask, in_off = run_verdict(emu, n, content_bytes, every, n, err_at=err_at, crc_at=crc_at)
        assert (st, enc) == (want, n) and not any(mask) and in_off == off, (err_at, crc_at)
    # a status from before stays, whatever the slots hold (nothing was decoded into them); a refused frame counts no block
    st, enc, mask, in_off = run_verdict(emu, n, content_bytes, every, n, err_at={3: E.EIO}, status=E.ENODATA)
    assert (st, enc) == (E.ENODATA, n) and not any(mask) and in_off == off
    st, enc, mask, in_off = run_verdict(emu, n, content_bytes, every[:4], 4, status=E.EINVAL, refused_frame=1)
    assert (st, enc) == (E.EINVAL, 0) and not any(mask) and in_off == [0] * 5


# ---------------------------------------------------------------------------------- the merge-index kernel
def small_content(n):
    """frames of 1 and 2 blocks, which frame_gather_cases has none of"""
    return {1: G.piece("t"), 2: G.piece("N") + G.piece("S")}[n]


def run_merge(em, old, content, version, touched, new_blocks, capacity=None, enc_err=None, status=0, m=None):
    """the kernel, then the splice over its table: the whole new frame but for index_crc"""
    n = (len(content) + BB - 1) // BB
    count = len(touched)
    m = count if m is None else m
    words = _bitmap(touched, n)
    bm, wpre = np.asarray(words + [0], np.uint32), _wpre(words)
    ctl = np.asarray([count, 0, 0], np.uint32)
    streams = [U.stream_of(b, 1 if version == 2 else version, False) for b in new_blocks]
    out_bytes = np.asarray([len(s) for s in streams] + [0], np.uint64)
    err = np.asarray((enc_err or [0] * count) + [0], np.int32)
    crc_new = np.asarray([zlib.crc32(b) for b in new_blocks] + [0], np.uint32)
    slabs, slots = aligned_copy(bytes(max(m, 1) * SLAB)), aligned_copy(bytes([0x5A]) * (max(m, 1) * BB))
    for k, (s, b) in enumerate(zip(streams, new_blocks)):
        slabs[k * SLAB:k * SLAB + len(s)] = np.frombuffer(s, np.uint8)
        slots[k * BB:k * BB + len(b)] = np.frombuffer(b, np.uint8)
    new = bytearray(content)
    for b, blk in zip(touched, new_blocks):
        new[b * BB:b * BB + len(blk)] = blk
    want = U.frame_of(bytes(new), version)
    capacity = len(want) if capacity is None else capacity
    frame = Arr(capacity, np.uint8, align=True)
    seg_dst, seg_src, seg_len = Arr(2 * m + 2, np.uint64), Arr(2 * m + 1, np.uint64), Arr(2 * m + 1, np.uint64)
    idx_off, fb, st = Arr(2, np.uint64), Arr(1, np.uint64), np.asarray([status], np.int32)
    buf = aligned_copy(old)
    em.emu_update_merge(_p(buf), n, u64(len(content)), 1 if version == 3 else 0, _p(bm), _p(wpre), _p(ctl), m,
                        _p(out_bytes), _p(err), _p(crc_new), u64(SLAB), _p(frame.a), u64(capacity), _p(seg_dst.a),
                        _p(seg_src.a), _p(seg_len.a), _p(idx_off.a), _p(fb.a), _p(st))
    assert all(a.guard_ok() for a in (frame, seg_dst, seg_src, seg_len, idx_off, fb))
    em.emu_update_splice(_p(buf), _p(slabs), _p(slots), _p(frame.a), _p(seg_dst.a), _p(seg_src.a), _p(seg_len.a), m,
                         u64(capacity))
    assert frame.guard_ok()
    return int(st[0]), int(fb.a[0]), frame, want, idx_off.a.tolist(), seg_dst.a.tolist()


def _same_but_for_the_seal(frame, want):
    got = bytearray(frame.a.tobytes())
    return bytes(got[:28]) + bytes(got[32:]) == want[:28] + want[32:] and got[28:32] == bytes(4)


@pytest.mark.parametrize("version", [1, 2, 3])
def test_merge_index_kernel_and_the_table_it_leaves(emu, version):
    cases = [(small_content(1), U.frame_of(small_content(1), version), "t"),
             (small_content(2), U.frame_of(small_content(2), version), "NS")]
    cases += [(G.content(k), G.frame(k, version), G.PATTERNS[k]) for k in ("mixed", "b70", "b300")]
    for content, old, pattern in cases:
        n = len(pattern)
        record = 8 if version == 3 else 0
        for touched in ([], [0], [n - 1], list(range(n)), [b for b in (0, 1, 31, 32, 33, 256, n - 2, n - 1) if 0 <= b < n]):
            touched = sorted(set(touched))
            # a touched block takes the letter of the other kind: text for noise, noise for text (the stored bit flips)
            new_blocks = [G.piece("t" if b == n - 1 and pattern[b] in "St" else "A" if pattern[b] == "N" else "N")
                          [:len(W.blocks_of(content, BITS)[b])] for b in touched]
            for m in {len(touched), len(touched) + 2}:
                st, fb, frame, want, idx_off, seg_dst = run_merge(emu, old, content, version, touched, new_blocks, m=m)
                what = (version, n, touched, m)
                assert (st, fb) == (0, len(want)), what
                assert _same_but_for_the_seal(frame, want), what
                assert idx_off == [32, 32 + 8 * n + record] and seg_dst == sorted(seg_dst) and seg_dst[-1] == len(want)
            # one byte short: E2BIG, the size it takes, and not one byte of the frame
            st, fb, frame, want, idx_off, seg_dst = run_merge(emu, old, content, version, touched, new_blocks,
                                                               capacity=len(want) - 1)
            assert (st, fb, idx_off) == (E.E2BIG, len(want), [0, 0]) and frame.untouched() and not any(seg_dst), what
            if touched:
                # an encoder errno: the first in ascending order, no size, nothing written
                bad = [0] * len(touched)
                bad[-1] = E.ENOBUFS
                if len(touched) > 1:
                    bad[0] = E.EINVAL
                st, fb, frame, *_ = run_merge(emu, old, content, version, touched, new_blocks, enc_err=bad)
                assert (st, fb) == (bad[0], 0) and frame.untouched(), what
            # a status from before: kept, and nothing is done
            st, fb, frame, want, idx_off, seg_dst = run_merge(emu, old, content, version, touched, new_blocks, status=E.ERANGE)
            assert (st, fb, idx_off) == (E.ERANGE, 0, [0, 0]) and frame.untouched() and not any(seg_dst)


# ---------------------------------------------------------------------------------- the whole chain
def run_update(em, frame, name, version, offsets, lengths, cap, max_blocks=None, data=None, data_bytes=None, dct=None,
               capacity=None, win_bits=WB, enc_err=None):
    content, n = G.content(name), len(G.PATTERNS[name])
    blocks = G.model(content, offsets, lengths, cap)[3]
    m = len(blocks) if max_blocks is None else max_blocks
    R, words = len(offsets), (n + 31) // 32
    o, ln = _ranges(offsets, lengths)
    if data is None:
        data, new_content = U.data_of(name, offsets, lengths, cap), U.patched(name, offsets, lengths, cap)
    else:                                                # the caller's own bytes (ranges that do not overlap)
        new_content, at = bytearray(content), 0
        for a, c in zip(offsets, lengths):
            if G.valid(a, c, cap, len(content)):
                new_content[a:a + c] = data[at:at + c]
                at += c
        new_content = bytes(new_content)
    want = U.frame_of(new_content, version)
    capacity = len(want) if capacity is None else capacity
    arrays = [Arr(words, np.uint32), Arr(words + 1, np.uint32), Arr(3, np.uint32), Arr(m, np.uint32),
              Arr(2 * m + 1, np.uint64), Arr(2 * m + 1, np.uint64), Arr(2 * m, np.uint32), Arr(2 * m, np.uint32),
              Arr(2 * m, np.uint32), Arr(2 * m, np.int32), Arr(R, np.uint64), Arr(R, np.uint32),
              Arr(m * BB + 64, np.uint32), Arr(2 * m, np.uint32), Arr(m * BB, np.uint8, align=True),
              Arr(R, np.uint64), Arr(m + 1, np.uint64), Arr(m + 1, np.uint64), Arr(m, np.uint64), Arr(m, np.int32),
              Arr(m, np.uint32), Arr(2 * m + 2, np.uint64), Arr(2 * m + 1, np.uint64), Arr(2 * m + 1, np.uint64),
              Arr(1, np.uint32), Arr(m * SLAB, np.uint8, align=True)]
    # what the encoder would leave: the oracle's streams of the patched blocks, by slot
    out_bytes, errs, slabs = arrays[18], arrays[19], arrays[25]
    guards = [a for k, a in enumerate(arrays) if k not in (18, 19, 25)]
    for k, b in enumerate(blocks[:m]):
        s = U.stream_of(new_content[b * BB:(b + 1) * BB], 1 if version == 2 else version, False)
        out_bytes.a[k] = len(s)
        errs.a[k] = 0 if enc_err is None else enc_err.get(b, 0)
        slabs.a[k * SLAB:k * SLAB + len(s)] = np.frombuffer(s, np.uint8)
    ptrs = (C.c_void_p * len(arrays))(*[a.a.ctypes.data for a in arrays])
    new = Arr(capacity, np.uint8, align=True)
    data_off, rerr = Arr(R + 1, np.uint64), Arr(R, np.int32)
    fb, enc, st = Arr(1, np.uint64), np.full(1, 0xDEAD, np.uint32), np.full(1, -1, np.int32)
    if version == 3 and dct is None:
        dct = G.dct()
    d = _dict(dct) if dct is not None else None
    buf, dbuf = aligned_copy(frame), aligned_copy(data + bytes(16))
    rc = em.emu_frame_update(_p(buf), u64(len(frame)), n, u64(len(content)), win_bits, BITS, _p(o), _p(ln), R, u64(cap), m,
                             _p(dbuf), u64(len(data) if data_bytes is None else data_bytes), _p(data_off.a), _p(d),
                             len(dct) if dct is not None else 0, _p(new.a), u64(capacity), _p(fb.a), _p(rerr.a), _p(enc),
                             _p(st), ptrs, u64(SLAB), 1 if cap > 4096 else 0)
    assert rc == 0
    assert all(a.guard_ok() for a in guards) and new.guard_ok() and data_off.guard_ok() and rerr.guard_ok() and fb.guard_ok()
    return {"status": int(st[0]), "encoded": int(enc[0]), "new": new, "frame_bytes": int(fb.a[0]), "want": want,
            "data_off": data_off.a.tolist(), "range_err": rerr.a.tolist(), "blocks": blocks, "slots": arrays[14], "err": arrays[9]}


def check_frame(got, what=None):
    assert (got["status"], got["frame_bytes"], got["encoded"]) == (0, len(got["want"]), len(got["blocks"])), what
    assert got["new"].a.tobytes() == got["want"], what


def refused(got, status, encoded=None, frame_bytes=0):
    assert (got["status"], got["frame_bytes"]) == (status, frame_bytes), (got["status"], got["frame_bytes"])
    assert encoded is None or got["encoded"] == encoded
    assert got["new"].untouched()
    return True


LISTS = ("one", "zero", "to_the_end", "two_edges", "last_block", "two_in_one_block", "descending", "unaligned", "whole")
CHAIN = [(v, name, LISTS) for name in ("mixed", "whole", "short") for v in (1, 2, 3)]
CHAIN += [(2, "b70", ("word_edges", "many_65")), (2, "b300", ("many_257",))]


@pytest.mark.parametrize("version,name,keys", CHAIN, ids=[f"v{v}-{n}" for v, n, _ in CHAIN])
def test_update_through_the_whole_chain(emu, version, name, keys):
    frame, content = G.frame(name, version), G.content(name)
    for key in keys:
        offsets, lengths, cap = G.range_lists(name)[key]
        got = run_update(emu, frame, name, version, offsets, lengths, cap)
        check_frame(got, (version, name, key))
        assert got["data_off"] == G.model(content, offsets, lengths, cap)[1] and not any(got["range_err"])


def test_no_range_copies_the_frame_and_a_wide_launch_changes_nothing(emu):
    for version in (1, 2, 3):
        frame = G.frame("short", version)
        got = run_update(emu, frame, "short", version, [], [], 0, max_blocks=4)
        check_frame(got)
        assert got["new"].a.tobytes() == frame and got["data_off"] == [0]
    offsets, lengths, cap = G.range_lists("short")["descending"]
    check_frame(run_update(emu, G.frame("short", 3), "short", 3, offsets, lengths, cap, max_blocks=4))
    # writing the content's own bytes back reproduces the old frame
    frame, content = G.frame("short", 2), G.content("short")
    data = b"".join(content[o:o + n] for o, n in zip(offsets, lengths))
    got = run_update(emu, frame, "short", 2, offsets, lengths, cap, data=data)
    assert got["status"] == 0 and got["new"].a[:got["frame_bytes"]].tobytes() == frame


def test_every_refusal_in_the_calls_order_writes_nothing(emu):
    name = "short"
    content = G.content(name)
    inv_o, inv_l, inv_cap = G.range_lists(name)["invalid"]
    o, ln, cap = G.range_lists(name)["descending"]
    count = len(G.model(content, o, ln, cap)[3])
    total = sum(ln)
    want_inv = [0, E.EINVAL, 0, E.EINVAL, 0, E.EINVAL, 0]
    for version in (2, 3):
        frame = G.frame(name, version)
        # 1. the frame's own status, in front of everything else
        wrong = dict(dct=G.dct()[:-1]) if version == 3 else dict(dct=G.dct())
        want = E.EILSEQ if version == 3 else E.EINVAL
        got = run_update(emu, frame, name, version, inv_o, inv_l, inv_cap, max_blocks=0, data_bytes=0, **wrong)
        assert refused(got, want, 0) and got["range_err"] == want_inv and got["slots"].untouched()
        assert got["data_off"] == G.model(content, inv_o, inv_l, inv_cap)[1]
        assert refused(run_update(emu, frame, name, version, o, ln, cap, win_bits=14), E.EINVAL, 0)
        # 2. ERANGE, in front of ENOBUFS and ENODATA; nothing is decoded
        got = run_update(emu, frame, name, version, inv_o, inv_l, inv_cap)
        assert refused(got, E.ERANGE) and got["range_err"] == want_inv and got["slots"].untouched()
        got = run_update(emu, frame, name, version, inv_o, inv_l, inv_cap, max_blocks=0, data_bytes=0)
        assert refused(got, E.ERANGE) and got["range_err"] == want_inv
        # 3. ENOBUFS with the distinct count, in front of ENODATA
        got = run_update(emu, frame, name, version, o, ln, cap, max_blocks=count - 1, data_bytes=total - 1)
        assert refused(got, E.ENOBUFS, count) and got["slots"].untouched() and not any(got["range_err"])
        # 4. ENODATA
        got = run_update(emu, frame, name, version, o, ln, cap, data_bytes=total - 1)
        assert refused(got, E.ENODATA, count) and got["slots"].untouched()
        # 5. a damaged touched block, in front of an encoder's errno and a capacity that would not do: the decoder's
        #    errno for that slot where it has one, else EILSEQ
        victim = 2
        entry = G.block_entries(frame, version)[victim]
        k = G.model(content, o, ln, cap)[3].index(victim)
        for at in (3, 9, entry["payload_bytes"] - 12):
            bad = bytearray(frame)
            bad[entry["payload_off"] + at] ^= 0x40
            got = run_update(emu, bytes(bad), name, version, o, ln, cap, enc_err={0: E.ENOBUFS}, capacity=64)
            slot_err = int(got["err"].a[2 * k])
            assert refused(got, slot_err if slot_err != 0 else E.EILSEQ, count), (version, at, slot_err)
        #    the stream as it was and an index entry with another CRC-32 (the index's own checksum made good): the
        #    decoder succeeds, so it is EILSEQ and nothing else
        bad = bytearray(frame)
        bad[32 + 8 * victim + 4] ^= 0x01
        index_end = 32 + 8 * len(G.PATTERNS[name]) + (8 if version == 3 else 0)
        bad[28:32] = zlib.crc32(bytes(bad[:28]) + bytes(bad[32:index_end])).to_bytes(4, "little")
        got = run_update(emu, bytes(bad), name, version, o, ln, cap, enc_err={0: E.ENOBUFS}, capacity=64)
        assert int(got["err"].a[2 * k]) == 0 and refused(got, E.EILSEQ, count)
        # 6. an encoder's errno, in front of the capacity
        got = run_update(emu, frame, name, version, o, ln, cap, enc_err={1: E.ENOBUFS, 2: E.EINVAL}, capacity=64)
        assert refused(got, E.ENOBUFS, count)
        # 7. E2BIG one byte short, with the size it takes
        need = len(U.frame_of(U.patched(name, o, ln, cap), version))
        assert refused(run_update(emu, frame, name, version, o, ln, cap, capacity=need - 1), E.E2BIG, count, need)
        check_frame(run_update(emu, frame, name, version, o, ln, cap, capacity=need))


def test_a_damaged_stored_touched_block_is_eilseq_and_a_damaged_kept_block_stays_as_it_is(emu):
    name, version = "short", 2                           # a N b t: block 1 is stored
    frame, content = G.frame(name, version), G.content(name)
    entries = G.block_entries(frame, version)
    assert entries[1]["stored"] == 1
    bad = bytearray(frame)
    bad[entries[1]["payload_off"] + 9] ^= 0x40
    got = run_update(emu, bytes(bad), name, version, [4100], [50], 50)           # touches block 1
    assert refused(got, E.EILSEQ, 1)
    # the same damage in a kept block: status 0, and the new frame is the expected one with that stream as damaged as
    # it was -- a decode of it blames exactly that block
    for o, ln in (([10, 8300], [20, 100]), ([8300], [100])):                     # touches blocks 0 and 2 / block 2
        got = run_update(emu, bytes(bad), name, version, o, ln, 100)
        assert got["status"] == 0 and got["frame_bytes"] == len(got["want"])
        want = bytearray(got["want"])
        want[G.block_entries(got["want"], version)[1]["payload_off"] + 9] ^= 0x40
        assert got["new"].a.tobytes() == bytes(want)
