"""CPU: many ranges of a resident frame in one call -- the mark, select, plan and copy kernels and the list flavour
of the open code (sqz_amd/csrc/frame.hip) with the decode kernels behind them (decode.hip) -- compiled by g++ against
tests/emu/hip/hip_runtime.h, run lane by lane on the CPU wave emulator and held against a few lines of Python over the
plain content (tests/frame_gather_cases.py).  This pins the kernels' LOGIC without a GPU; the -m gpu tests
(test_frame_gather_gpu.py) pin the gfx950 build.

The emulator takes seconds to decode a 4 KB stream of noise, which versions 2 and 3 store: version 1 runs over the
three-block content with the lists that matter there, the long frames as versions 2 and 3."""
import ctypes as C
import errno
import os
import struct
import subprocess

import numpy as np
import pytest

import frame_gather_cases as G
import frame_writer_v3 as W3
from test_frame_emu import aligned_copy
from test_frame_v3_emu import _refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
E = errno
GUARD = 8                       # entries behind every array
FILL = 0xA5
BB, BITS = G.BB, G.BITS


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU, "libsqz_emu_frame_gather.so")
    deps = [os.path.join(EMU, f) for f in ("emu_runtime.cpp", "emu_frame_gather.cpp", "hip/hip_runtime.h")] + \
           [os.path.join(CSRC, f) for f in ("frame.hip", "decode.hip", "sqz_tree.h", "sqz_device.h", "sqz_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-I" + EMU,
                               "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                               "-Wno-attributes", os.path.join(EMU, "emu_runtime.cpp"),
                               os.path.join(EMU, "emu_frame_gather.cpp"), "-o", out])
    return C.CDLL(out)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def u64(v):
    return C.c_uint64(v)


class Arr:
    """an array the kernels write, with GUARD entries of a pattern behind it"""

    def __init__(self, n, dtype, align=False):
        self.n = n
        self.fill = np.frombuffer(bytes([FILL]) * 8, dtype)[0]
        raw = np.full(n + GUARD + (16 if align else 0), self.fill, dtype)
        self.all = raw[(-raw.ctypes.data) % 16 // raw.itemsize:][:n + GUARD] if align else raw
        self.a = self.all[:n]

    def guard_ok(self):
        return bool((self.all[self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.all == self.fill).all())


def _ranges(offsets, lengths):
    return np.asarray(list(offsets) + [0], np.uint64), np.asarray(list(lengths) + [0], np.uint64)


def _bitmap(blocks, n):
    words = [0] * ((n + 31) // 32)
    for b in blocks:
        words[b >> 5] |= 1 << (b & 31)
    return words


def _dict(d: bytes):
    return np.frombuffer(d + bytes(16), np.uint8).copy()


def test_the_shared_inputs_are_what_they_are_there_for():
    G.check_layout()


# ---------------------------------------------------------------------------------- mark and select
def run_mark(em, name, offsets, lengths, cap):
    data, n = G.content(name), len(G.PATTERNS[name])
    o, ln = _ranges(offsets, lengths)
    bitmap = Arr((n + 31) // 32, np.uint32)
    em.emu_gather_mark(_p(o), _p(ln), len(offsets), u64(cap), u64(len(data)), BITS, n, _p(bitmap.a))
    assert bitmap.guard_ok()
    return bitmap.a.tolist()


def test_mark_kernel_sets_the_covering_blocks_bits_and_no_other(emu):
    for name in G.PATTERNS:
        data, n = G.content(name), len(G.PATTERNS[name])
        for key, (offsets, lengths, cap) in G.range_lists(name).items():
            blocks = G.model(data, offsets, lengths, cap)[3]
            assert run_mark(emu, name, offsets, lengths, cap) == _bitmap(blocks, n), (name, key)
    # a range of every block of the longest frame: whole words in the middle, part words at both ends
    n = 300
    assert run_mark(emu, "b300", [BB + 5], [len(G.content("b300")) - BB - 5], 1 << 30) == _bitmap(range(1, n), n)
    assert run_mark(emu, "b300", [], [], 0) == [0] * 10


def run_select(em, name, offsets, lengths, cap, max_blocks, out_capacity, bitmap=None):
    data, n = G.content(name), len(G.PATTERNS[name])
    words = (n + 31) // 32
    blocks = G.model(data, offsets, lengths, cap)[3]
    bm = np.asarray((_bitmap(blocks, n) if bitmap is None else bitmap) + [0], np.uint32)
    o, ln = _ranges(offsets, lengths)
    wpre, sel, ctl = Arr(words + 1, np.uint32), Arr(max_blocks, np.uint32), Arr(2, np.uint32)
    out_off = Arr(len(offsets) + 1, np.uint64)
    em.emu_gather_select(_p(bm), n, _p(o), _p(ln), len(offsets), u64(cap), u64(len(data)), max_blocks,
                         u64(out_capacity), _p(wpre.a), _p(sel.a), _p(out_off.a), _p(ctl.a))
    assert wpre.guard_ok() and sel.guard_ok() and ctl.guard_ok() and out_off.guard_ok()
    return wpre.a.tolist(), sel, out_off.a.tolist(), ctl.a.tolist()


def test_select_kernel_list_prefix_counts_layout_and_verdicts(emu):
    for name in G.PATTERNS:
        data, n = G.content(name), len(G.PATTERNS[name])
        for key, (offsets, lengths, cap) in G.range_lists(name).items():
            _, want_off, _, blocks = G.model(data, offsets, lengths, cap)
            count, total, what = len(blocks), want_off[-1], (name, key)
            words = _bitmap(blocks, n)
            want_pre = [sum(bin(w).count("1") for w in words[:k]) for k in range(len(words) + 1)]
            # max_blocks equal to the count, and anything above it
            for m in (count, count + 3, n):
                wpre, sel, out_off, ctl = run_select(emu, name, offsets, lengths, cap, m, total)
                assert (wpre, out_off, ctl) == (want_pre, want_off, [count, 0]), what
                assert sel.a[:count].tolist() == blocks and (sel.a[count:] == sel.fill).all(), what
            # one block less than it takes: ENOBUFS, the list cut at the cap, the layout as it was
            if count > 0:
                wpre, sel, out_off, ctl = run_select(emu, name, offsets, lengths, cap, count - 1, total)
                assert (wpre, out_off, ctl) == (want_pre, want_off, [count, E.ENOBUFS]), what
                assert sel.a.tolist() == blocks[:count - 1], what
            # one byte less than it takes: ENOSPC; both at once: ENOBUFS
            if total > 0:
                assert run_select(emu, name, offsets, lengths, cap, count, total - 1)[3] == [count, E.ENOSPC], what
                if count > 0:
                    assert run_select(emu, name, offsets, lengths, cap, count - 1, 0)[3] == [count, E.ENOBUFS], what
    # lengths that add up to more than 64 bits hold (the content is what the caller says it is): ENOSPC, no wrap
    big = 1 << 63
    o, ln = _ranges([0, 0, 0], [big, big, 5])
    wpre, sel, ctl, out_off = Arr(2, np.uint32), Arr(1, np.uint32), Arr(2, np.uint32), Arr(4, np.uint64)
    emu.emu_gather_select(_p(np.zeros(2, np.uint32)), 1, _p(o), _p(ln), 3, u64(big), u64(big), 1, u64(G.M64),
                          _p(wpre.a), _p(sel.a), _p(out_off.a), _p(ctl.a))
    assert ctl.a.tolist() == [0, E.ENOSPC] and out_off.a[:2].tolist() == [0, big]


# ---------------------------------------------------------------------------------- the open kernel, for a list
def run_open(em, frame, n, content, dct, blocks, max_blocks, verdict=0, avail=None, want_bits=BITS, sel_blocks=None):
    buf = aligned_copy(frame)
    words = _bitmap(blocks, n)
    bm = np.asarray(words + [0], np.uint32)
    wpre = np.asarray([sum(bin(w).count("1") for w in words[:k]) for k in range(len(words) + 1)], np.uint32)
    sel = np.asarray(list(blocks)[:max_blocks] + [0], np.uint32)
    ctl = np.asarray([len(blocks), verdict], np.uint32)
    in_off, out_off = Arr(2 * max_blocks + 1, np.uint64), Arr(2 * max_blocks + 1, np.uint64)
    skip, stored = Arr(2 * max_blocks, np.uint32), Arr(2 * max_blocks, np.uint32)
    st, dec = np.full(1, -1, np.int32), np.full(1, 0xDEAD, np.uint32)
    d = _dict(dct) if dct is not None else None
    rc = em.emu_gather_open(_p(buf), u64(len(frame) if avail is None else avail), n, u64(content), _p(d),
                            len(dct) if dct is not None else 0, _p(bm), _p(wpre), _p(sel), _p(ctl), max_blocks,
                            _p(in_off.a), _p(out_off.a), _p(skip.a), _p(stored.a), _p(st), _p(dec), want_bits)
    assert in_off.guard_ok() and out_off.guard_ok() and skip.guard_ok() and stored.guard_ok()
    return rc, int(st[0]), int(dec[0]), in_off.a.tolist(), out_off.a.tolist(), skip.a.tolist(), stored.a.tolist()


def _empty(in_off, out_off, skip, stored, start=0):
    return (len(set(in_off[start:])) <= 1 and len(set(out_off[start:])) <= 1 and all(skip[start:])
            and not any(stored[start:]))


@pytest.mark.parametrize("version", [1, 2, 3])
def test_open_kernel_builds_two_entries_per_slot(emu, version):
    for name in G.PATTERNS:
        frame, data, n = G.frame(name, version), G.content(name), len(G.PATTERNS[name])
        entries = G.block_entries(frame, version)
        dct = G.dct() if version == 3 else None
        picks = [[], [0], [n - 1], [0, n - 1], list(range(n)), list(range(0, n, 2)), [b for b in G.EDGES if b < n]]
        for blocks in picks:
            count = len(blocks)
            for m in {count, count + 2, n}:
                rc, st, dec, in_off, out_off, skip, stored = run_open(emu, frame, n, len(data), dct, blocks, m)
                assert (rc, st, dec) == (0, 0, count), (name, blocks, m)
                for k, b in enumerate(blocks):
                    e = entries[b]
                    assert in_off[2 * k:2 * k + 2] == [e["payload_off"], e["payload_off"] + e["payload_bytes"]]
                    assert out_off[2 * k:2 * k + 2] == [k * BB, k * BB + e["content_bytes"]]
                    assert (skip[2 * k], skip[2 * k + 1], stored[2 * k], stored[2 * k + 1]) == (e["stored"], 1, e["stored"], 0)
                # monotone, so that no entry has a negative length; and the slots behind the count are empty
                assert in_off == sorted(in_off) and out_off == sorted(out_off)
                assert in_off[2 * count:] == [len(frame)] * (2 * (m - count) + 1)
                assert _empty(in_off, out_off, skip, stored, 2 * count), (name, blocks, m)
            # a cap that did not hold: the verdict is the status, the count is reported, nothing is selected
            if count > 0:
                for verdict in (E.ENOBUFS, E.ENOSPC):
                    rc, st, dec, in_off, out_off, skip, stored = run_open(emu, frame, n, len(data), dct, blocks,
                                                                          count - 1, verdict)
                    assert (rc, st, dec) == (0, verdict, count) and _empty(in_off, out_off, skip, stored)
                    assert not any(in_off) and not any(out_off)


def test_open_kernel_refusals_in_the_hosts_order(emu):
    """the refusals of the version-3 open kernel (test_frame_v3_emu.py), through the list flavour: the same status,
    no block counted, every entry empty and skipped -- and before the verdict on the caps"""
    dct, data = G.dct(), G.content("mixed")
    store_frame = G.frame("mixed", 3)
    plain_frame = W3.assemble(data, G.WB, BITS, dct, [G._stream(c, 3, False) for c in "ANS"], store=False)
    seen = set()
    for what, bad, d, content, want in _refusals(store_frame, plain_frame, data, dct):
        for verdict in (0, E.ENOBUFS):
            rc, st, dec, in_off, out_off, skip, stored = run_open(emu, bad, 3, content, d, [0, 2], 3, verdict)
            assert (rc, st, dec) == (0, want, 0), (what, st)
            assert not any(in_off) and not any(out_off) and _empty(in_off, out_off, skip, stored), what
        seen.add(want)
    assert seen == {E.EINVAL, E.EILSEQ}
    rc, st, dec, in_off, *_ = run_open(emu, store_frame, 3, len(data), dct, [1], 1, avail=len(store_frame) - 8)
    assert (rc, st, dec) == (0, E.E2BIG, 0) and not any(in_off)
    assert run_open(emu, store_frame, 3, len(data), dct[:-1], [1], 1, avail=len(store_frame) - 8)[1] == E.EILSEQ
    assert run_open(emu, store_frame, 3, len(data), dct, [1], 1, avail=32 + 24 + 7)[0] == E.E2BIG    # at the call
    assert run_open(emu, store_frame, 3, len(data), dct, [1], 1, want_bits=13)[1:3] == (E.EINVAL, 0)
    # versions 1 and 2 through the flavour without a dictionary, which refuses version 3 and is refused by the other
    for version in (1, 2):
        frame = G.frame("mixed", version)
        assert run_open(emu, frame, 3, len(data), None, [1], 1)[1:3] == (0, 1)
        assert run_open(emu, frame, 3, len(data), None, [1], 1, want_bits=13)[1:3] == (E.EINVAL, 0)
        assert run_open(emu, frame, 3, len(data), None, [1], 1, avail=len(frame) - 8)[1:3] == (E.E2BIG, 0)
        assert run_open(emu, frame, 3, len(data) - 1, None, [1], 1)[1:3] == (E.EINVAL, 0)
        assert run_open(emu, frame, 3, len(data), dct, [1], 1)[1:3] == (E.EINVAL, 0)
        bad = bytearray(frame)
        bad[32 + 8 + 5] ^= 0x10
        assert run_open(emu, bytes(bad), 3, len(data), None, [1], 1)[1:3] == (E.EILSEQ, 0)
    assert run_open(emu, store_frame, 3, len(data), None, [1], 1)[1:3] == (E.EINVAL, 0)


# ---------------------------------------------------------------------------------- the plan kernel
def test_plan_kernel_range_errors_and_work_list(emu):
    name = "b70"
    data, n, frame = G.content(name), 70, aligned_copy(G.frame(name, 3))
    index = [b["content_crc"] for b in G.block_entries(G.frame(name, 3), 3)]
    for key, (offsets, lengths, cap) in G.range_lists(name).items():
        parts, out_off, want_err, blocks = G.model(data, offsets, lengths, cap)
        slot = {b: k for k, b in enumerate(blocks)}
        words = _bitmap(blocks, n)
        bm = np.asarray(words + [0], np.uint32)
        wpre = np.asarray([sum(bin(w).count("1") for w in words[:k]) for k in range(len(words) + 1)], np.uint32)
        o, ln = _ranges(offsets, lengths)
        R = len(offsets)

        def run(status, bad=(), bad_crc=()):
            err, crc = np.full(2 * len(blocks) + 2, 77, np.int32), np.full(2 * len(blocks) + 2, 0x77777777, np.uint32)
            for b, k in slot.items():
                err[2 * k] = bad[b] if b in bad else 0
                crc[2 * k] = index[b] ^ (1 if b in bad_crc else 0)
            rerr, src, mask = Arr(R, np.int32), Arr(R, np.uint64), Arr(R, np.uint32)
            emu.emu_gather_plan(_p(frame), _p(o), _p(ln), R, u64(cap), u64(len(data)), BITS, n, _p(bm), _p(wpre), _p(err),
                                _p(crc), _p(np.asarray([status], np.int32)), _p(rerr.a), _p(src.a), _p(mask.a))
            assert rerr.guard_ok() and src.guard_ok() and mask.guard_ok()
            return rerr.a.tolist(), src.a.tolist(), mask.a.tolist()

        rerr, src, mask = run(0)
        assert rerr == want_err, key
        assert mask == [1 if p else 0 for p in parts], key                   # (an empty range has nothing to copy)
        for r, p in enumerate(parts):
            if p:
                assert src[r] == slot[offsets[r] >> BITS] * BB + offsets[r] % BB, (key, r)
        # the call's status goes to every valid range, and nothing is delivered
        rerr, src, mask = run(E.ENOSPC)
        assert rerr == [E.ENOSPC if e == 0 else e for e in want_err] and not any(mask), key
        # a block the decoder refused, one whose bytes are not the checksummed ones: the first in ascending order
        if len(blocks) >= 2:
            b0, b1 = blocks[0], blocks[1]
            rerr, src, mask = run(0, bad={b1: E.E2BIG}, bad_crc={b0})
            for r, (a, c) in enumerate(zip(offsets, lengths)):
                if want_err[r] == 0:
                    cov = list(G.covering(a, c))
                    want = E.EILSEQ if b0 in cov else E.E2BIG if b1 in cov else 0
                    assert rerr[r] == want and mask[r] == (1 if want == 0 and c > 0 else 0), (key, r)


# ---------------------------------------------------------------------------------- the copy kernels
@pytest.mark.parametrize("wide", [0, 1])
def test_copy_kernels_move_the_same_work_lists(emu, wide):
    """gather_copy_kernel (wide = 0) and range_copy_kernel on one work list: every alignment of source against
    destination, lengths around the 16-byte row, ranges left out by the mask, nothing outside a destination range"""
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, 70000, dtype=np.uint8)
    lengths = [0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 255, 256, 257, 300, 4095, 4096, 4099]
    for shift in range(0, 16, 3):
        lens = lengths * 2
        src_off = np.asarray([(37 * k * k + shift * (k + 1)) % 60000 for k in range(len(lens))] + [0], np.uint64)
        mask = np.asarray([0 if k % 7 == 3 else 1 for k in range(len(lens))] + [1], np.uint32)
        off = np.cumsum([0] + lens).astype(np.uint64)
        total = int(off[-1])
        dst = Arr(total + shift, np.uint8, align=True)
        emu.emu_gather_copy(_p(src), _p(src_off), _p(dst.a[shift:]), _p(off), _p(off), _p(mask), len(lens), wide, u64(max(lens)))
        assert dst.guard_ok() and (dst.a[:shift] == FILL).all()
        for k, n in enumerate(lens):
            got = dst.a[shift + int(off[k]):shift + int(off[k]) + n]
            if mask[k]:
                assert got.tobytes() == src[int(src_off[k]):int(src_off[k]) + n].tobytes(), (shift, k, n)
            else:
                assert (got == FILL).all(), (shift, k, n)
    # more ranges than a workgroup has groups of lanes, in an order that is not the destination's
    count = 100
    src_off = np.asarray([(count - k) * 200 + k % 5 for k in range(count)] + [0], np.uint64)
    off = np.arange(count + 1, dtype=np.uint64) * 131
    dst = Arr(131 * count, np.uint8, align=True)
    emu.emu_gather_copy(_p(src), _p(src_off), _p(dst.a), _p(off), _p(off), None, count, wide, u64(131))
    want = b"".join(src[int(s):int(s) + 131].tobytes() for s in src_off[:count])
    assert dst.guard_ok() and dst.a.tobytes() == want


# ---------------------------------------------------------------------------------- the whole chain
def run_gather(em, frame, name, version, offsets, lengths, cap, max_blocks=None, out_capacity=None, dct=None, wide=0,
               waves=1):
    data, n = G.content(name), len(G.PATTERNS[name])
    parts, want_off, _, blocks = G.model(data, offsets, lengths, cap)
    m = len(blocks) if max_blocks is None else max_blocks
    total = want_off[-1]
    out_capacity = total if out_capacity is None else out_capacity
    R, words = len(offsets), (n + 31) // 32
    o, ln = _ranges(offsets, lengths)
    arrays = [Arr(words, np.uint32), Arr(words + 1, np.uint32), Arr(2, np.uint32), Arr(m, np.uint32),
              Arr(2 * m + 1, np.uint64), Arr(2 * m + 1, np.uint64), Arr(2 * m, np.uint32), Arr(2 * m, np.uint32),
              Arr(2 * m, np.uint32), Arr(2 * m, np.int32), Arr(R, np.uint64), Arr(R, np.uint32),
              Arr(m * BB + 64, np.uint32), Arr(2 * m, np.uint32), Arr(m * BB, np.uint8, align=True)]
    ptrs = (C.c_void_p * len(arrays))(*[a.a.ctypes.data for a in arrays])
    out, out_off, rerr = Arr(out_capacity, np.uint8, align=True), Arr(R + 1, np.uint64), Arr(R, np.int32)
    dec, st = np.full(1, 0xDEAD, np.uint32), np.full(1, -1, np.int32)
    if version == 3 and dct is None:
        dct = G.dct()
    d = _dict(dct) if dct is not None else None
    buf = aligned_copy(frame)
    rc = em.emu_frame_gather(_p(buf), u64(len(frame)), n, u64(len(data)), BITS, _p(o), _p(ln), R, u64(cap), m, _p(d),
                             len(dct) if dct is not None else 0, _p(out.a), u64(out_capacity), _p(out_off.a),
                             _p(rerr.a), _p(dec), _p(st), ptrs, waves, wide)
    assert rc == 0
    assert all(a.guard_ok() for a in arrays) and out.guard_ok() and out_off.guard_ok() and rerr.guard_ok()
    return {"status": int(st[0]), "decoded": int(dec[0]), "out": out, "out_off": out_off.a.tolist(),
            "range_err": rerr.a.tolist(), "sel": arrays[3], "blocks": arrays[14]}


def check_delivery(got, data, offsets, lengths, cap, bad_blocks=(), bad_errno=E.EILSEQ, what=None):
    parts, want_off, want_err, blocks = G.model(data, offsets, lengths, cap, bad_blocks, bad_errno)
    assert got["status"] == 0 and got["decoded"] == len(blocks), what
    assert got["out_off"] == want_off and got["range_err"] == want_err, what
    assert got["sel"].a[:len(blocks)].tolist() == blocks and (got["sel"].a[len(blocks):] == got["sel"].fill).all(), what
    out = got["out"].a
    for r, p in enumerate(parts):
        piece = out[want_off[r]:want_off[r + 1]]
        if p is None:
            assert (piece == FILL).all(), (what, r)                  # a range that is not delivered is not written
        else:
            assert piece.tobytes() == p, (what, r)


# The emulator takes 2 s for a 4 KB block of text and 0.1 s for one of the blocks the long frames are made of.  The
# three-block content of text, noise and text runs the lists that differ in which of its blocks they cover (version 1,
# whose noise is a stream of seconds, those that keep to the others), the long frames the lists made for them and
# some of the random ones; mark, select and plan above have run every list of every frame.
CHAIN = [(1, "mixed", ("two_in_one_block", "last_block", "zero")),
         (2, "mixed", ("one", "to_the_end", "invalid")),
         (3, "mixed", ("one", "two_edges", "last_block", "unaligned", "descending", "many_65")),
         (2, "whole", ("one", "to_the_end", "two_edges", "whole")), (3, "short", None),
         (1, "short", ("zero", "last_block", "twice")),
         (2, "b70", ("word_edges", "many_64")), (3, "b70", ("word_edges", "many_63", "many_255")),
         (2, "b300", ("word_edges", "many_256")), (3, "b300", ("word_edges", "many_65", "many_257"))]


@pytest.mark.parametrize("version,name,keys", CHAIN, ids=[f"v{v}-{n}" for v, n, _ in CHAIN])
def test_gather_through_the_whole_chain(emu, version, name, keys):
    frame, data = G.frame(name, version), G.content(name)
    for key, (offsets, lengths, cap) in G.range_lists(name).items():
        if keys is not None and key not in keys or key == "whole" and len(G.PATTERNS[name]) > 4:
            continue
        wide = 1 if cap > 4096 else 0                                # the library's switch
        got = run_gather(emu, frame, name, version, offsets, lengths, cap, wide=wide)
        check_delivery(got, data, offsets, lengths, cap, what=(version, name, key))


def test_one_range_is_the_ranged_reads_bytes_whichever_copy_moves_it(emu):
    frame, data = G.frame("short", 3), G.content("short")
    for at, n in ((4090, 12), (8000, 400), (8500, 596), (0, len(data)), (len(data) - 1, 1)):
        for wide in (0, 1):
            got = run_gather(emu, frame, "short", 3, [at], [n], n, wide=wide)
            check_delivery(got, data, [at], [n], n, what=(at, n, wide))
    # the decode launch wider than the count, and more waves per stream
    frame, data = G.frame("mixed", 3), G.content("mixed")
    offsets, lengths, cap = G.range_lists("mixed")["descending"]
    for waves in (1, 4):
        got = run_gather(emu, frame, "mixed", 3, offsets, lengths, cap, max_blocks=3, waves=waves)
        check_delivery(got, data, offsets, lengths, cap)
    got = run_gather(emu, G.frame("b70", 3), "b70", 3, [5], [7], 7, max_blocks=70)
    check_delivery(got, G.content("b70"), [5], [7], 7)
    got = run_gather(emu, frame, "mixed", 3, [], [], 0, max_blocks=3)      # no range at all: the frame's status
    assert (got["status"], got["decoded"], got["out_off"]) == (0, 0, [0])


def test_the_caps_hold_and_say_what_to_ask_for(emu):
    for version, name, key in ((3, "short", "descending"), (2, "b70", "word_edges"), (3, "b300", "many_63")):
        frame, data = G.frame(name, version), G.content(name)
        offsets, lengths, cap = G.range_lists(name)[key]
        parts, want_off, want_err, blocks = G.model(data, offsets, lengths, cap)
        count, total = len(blocks), want_off[-1]
        # exactly enough of both
        check_delivery(run_gather(emu, frame, name, version, offsets, lengths, cap, count, total), data, offsets, lengths, cap)
        for m, capacity, want in ((count - 1, total, E.ENOBUFS), (count, total - 1, E.ENOSPC), (count - 1, total - 1, E.ENOBUFS)):
            got = run_gather(emu, frame, name, version, offsets, lengths, cap, m, capacity)
            assert (got["status"], got["decoded"]) == (want, count), (name, m, capacity)
            assert got["out_off"] == want_off and got["range_err"] == [want if e == 0 else e for e in want_err]
            assert got["out"].untouched() and got["blocks"].untouched()          # nothing decoded, nothing delivered
            assert got["sel"].a.tolist() == blocks[:m]
    # invalid ranges keep their EINVAL under a cap that did not hold
    offsets, lengths, cap = G.range_lists("short")["invalid"]
    got = run_gather(emu, G.frame("short", 3), "short", 3, offsets, lengths, cap, out_capacity=3)
    assert got["status"] == E.ENOSPC and got["range_err"] == [E.ENOSPC, E.EINVAL, E.ENOSPC, E.EINVAL, E.ENOSPC, E.EINVAL, E.ENOSPC]


def test_a_damaged_block_costs_the_ranges_that_touch_it_and_nothing_else(emu):
    for version, name, key, victim in ((3, "mixed", "unaligned", 2), (2, "b70", "word_edges", 32),
                                       (3, "b70", "word_edges", 31), (2, "short", "descending", 1)):
        frame, data = G.frame(name, version), G.content(name)
        offsets, lengths, cap = G.range_lists(name)[key]
        bad = bytearray(frame)
        entry = G.block_entries(frame, version)[victim]
        bad[entry["payload_off"] + 9] ^= 0x40
        got = run_gather(emu, bytes(bad), name, version, offsets, lengths, cap, wide=1 if cap > 4096 else 0)
        size = len(data)
        errs = {e for e, (a, c) in zip(got["range_err"], zip(offsets, lengths))
                if G.valid(a, c, cap, size) and victim in G.covering(a, c)}
        assert len(errs) == 1 and 0 not in errs, (name, key)         # a stored block: EILSEQ; a stream: the decoder's or EILSEQ
        check_delivery(got, data, offsets, lengths, cap, {victim}, errs.pop(), what=(name, key))
        assert entry["stored"] == (1 if G.PATTERNS[name][victim] == "N" else 0)


def test_a_refused_frame_delivers_nothing_but_the_layout(emu):
    name = "short"
    data = G.content(name)
    offsets, lengths, cap = G.range_lists(name)["invalid"]
    want_off = G.model(data, offsets, lengths, cap)[1]
    cases = [(3, G.frame(name, 3), G.dct()[:-1], E.EILSEQ),              # a wrong dictionary
             (2, G.frame(name, 3), None, E.EINVAL),                      # version 3 without one
             (3, G.frame(name, 2), G.dct(), E.EINVAL)]                   # version 2 with one
    torn = bytearray(G.frame(name, 2))
    struct.pack_into("<Q", torn, 16, struct.unpack_from("<Q", torn, 16)[0] + 8)
    cases.append((2, bytes(torn), None, E.EILSEQ))
    for version, frame, dct, want in cases:
        got = run_gather(emu, frame, name, version, offsets, lengths, cap, dct=dct)
        assert (got["status"], got["decoded"]) == (want, 0)
        assert got["out_off"] == want_off and got["out"].untouched() and got["blocks"].untouched()
        assert got["range_err"] == [want, E.EINVAL, want, E.EINVAL, want, E.EINVAL, want]
        # ... and the frame's status comes before a cap that would not hold either
        got = run_gather(emu, frame, name, version, offsets, lengths, cap, max_blocks=0, out_capacity=0, dct=dct)
        assert (got["status"], got["decoded"]) == (want, 0) and got["out_off"] == want_off
