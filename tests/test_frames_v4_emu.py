"""CPU: the kernels of a batch with byte-shuffled (version 4) frames in it -- the shuffle kernel for ranges of mixed
element size (sqz_amd/csrc/shuffle.hip) and the version-4 flavours of the batch's scan, plan, index and open kernels
(sqz_amd/csrc/frame.hip) -- compiled by g++ against tests/emu/hip/hip_runtime.h, each run by itself lane by lane on
the CPU wave emulator with guard values behind every array, and held against numpy, the independent writers
(tests/frame_writer*.py) and formulas written out in tests/frames_v4_cases.py.  This pins the kernels' LOGIC, every
alignment and every byte they may not touch, without a GPU; the -m gpu tests pin the gfx950 build."""
import ctypes as C
import errno
import os
import subprocess

import numpy as np
import pytest

import frame_gather_cases as G
import frame_writer as W
import frame_writer_v2 as W2
import frame_writer_v4 as W4
import frames_v4_cases as V
from test_frame_emu import LENGTHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
TILE_BYTES = 8192                                            # kShufTile
GUARD = 0xA5
G64, G32 = 0x7777777777777777, 0x77777777
STORED = 1
WB, BITS, BB = V.WB, V.BITS, V.BB
ITEM = np.dtype([("frame_at", "<u8"), ("avail", "<u8"), ("content_bytes", "<u8"), ("out_at", "<u8"),
                 ("n_blocks", "<u4"), ("zero", "<u4")])


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(EMU, "libsqz_emu_frames_v4.so")
    deps = [os.path.join(EMU, f) for f in ("emu_runtime.cpp", "emu_frames_v4.cpp", "hip/hip_runtime.h")] + \
           [os.path.join(CSRC, f) for f in ("frame.hip", "shuffle.hip", "sqz_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-I" + EMU,
                               "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                               "-Wno-attributes", os.path.join(EMU, "emu_runtime.cpp"),
                               os.path.join(EMU, "emu_frames_v4.cpp"), "-o", out])
    return C.CDLL(out)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def aligned(n, fill=GUARD):
    raw = np.full(n + 16, fill, np.uint8)
    return raw[(-raw.ctypes.data) % 16:][:n]


# ---------------------------------------------------------------------------------- the shuffle of mixed ranges
PATTERN = np.random.default_rng(23).integers(0, 256, 1 << 20, dtype=np.uint8)
MIS = (0, 1, 7, 16)


def lengths_for(e):
    t = TILE_BYTES // max(e, 1)                              # one below, at and above the tile, in elements
    w = max(e, 1)
    tile = [(t - 1) * w, t * w, (t + 1) * w, t * w + w - 1] if e else [TILE_BYTES - 16, TILE_BYTES, TILE_BYTES + 17]
    return sorted(set(LENGTHS + list(range(2 * w + 2)) + tile))


def transform(blk: bytes, e: int, inverse: bool):
    """what range of element size e becomes: None = left alone"""
    if e == 0:
        return blk
    if e in (2, 4, 8):
        return W4.unshuffle(blk, e) if inverse else W4.shuffle(blk, e)
    return None


def run_ranges(em, inverse, specs, src_mis, dst_mis, hint=None, call="ranges", front=5):
    """specs: [(gap in front, length, elem, skip)]; the first range starts `front` bytes behind a base that is misaligned
    by src_mis in the source and dst_mis in the destination.  Gaps are ranges of their own, switched off.  Checks every
    byte of the destination: the ranges' against numpy, the guard bytes in front of, between and behind them."""
    cuts, elem, mask = [front], [], []
    for gap, n, e, skip in specs:
        if gap:
            cuts.append(cuts[-1] + gap)
            elem.append(4)                                   # (a gap that was not switched off would be shuffled)
            mask.append(1)
        cuts.append(cuts[-1] + n)
        elem.append(e)
        mask.append(1 if skip else 0)
    end = cuts[-1]
    src, dst = aligned(end + 64, 0), aligned(end + 64)
    src[:] = PATTERN[:len(src)]
    sb, db = src[src_mis:], dst[dst_mis:]
    off = np.asarray(cuts, np.uint64)
    el, m = np.asarray(elem + [G32], np.uint32), np.asarray(mask + [G32], np.uint32)
    n = len(elem)
    if hint is None:
        hint = max([b - a for a, b in zip(cuts, cuts[1:])] + [1])
    if call == "ranges":
        em.emu_shuffle_ranges(_p(sb), _p(off), _p(el), n, int(inverse), _p(db), _p(m) if any(mask) else None,
                              C.c_uint64(hint))
    else:                                                    # the kernel of one element size, on a uniform batch
        em.emu_shuffle_blocks(_p(sb), _p(off), n, call, int(inverse), _p(db), _p(m) if any(mask) else None,
                              C.c_uint64(hint))
    want = np.full(len(dst), GUARD, np.uint8)
    for a, b, e, masked in zip(cuts, cuts[1:], elem, mask):
        got = None if masked else transform(sb[a:b].tobytes(), e, inverse)
        if got is not None:
            want[dst_mis + a:dst_mis + b] = np.frombuffer(got, np.uint8)
    bad = np.nonzero(dst != want)[0]
    assert bad.size == 0, (inverse, specs[:6], src_mis, dst_mis, hint, call, bad[:8].tolist())
    assert el[n] == G32 and m[n] == G32
    return dst


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("e", [0, 2, 4, 8])
def test_every_length_between_neighbours_of_other_element_sizes(emu, e, inverse):
    # range j has the j-th length of lengths_for(e) and element size e; its neighbours have the others, 0 included, and
    # touch it (gap 0) or stand off by an odd gap
    others = [x for x in (0, 2, 4, 8) if x != e]
    specs = []
    for j, n in enumerate(lengths_for(e)):
        specs.append((0 if j % 2 else 3, 1 + 37 * (j % 5), others[j % 3], False))
        specs.append((0, n, e, False))
    specs.append((1, 300, others[0], False))
    for s in MIS:
        for d in MIS:
            run_ranges(emu, inverse, specs, s, d)


@pytest.mark.parametrize("inverse", [False, True])
def test_a_long_range_shared_by_several_workgroups_and_a_skip_mask(emu, inverse):
    long = 3 * TILE_BYTES + 7 * 8 + 5                        # three tiles and a ragged part, for every element size
    specs = [(0, 5, 2, False), (0, long, 8, False), (2, long, 0, False), (0, 4096, 4, True), (0, long, 2, False),
             (7, 0, 4, False), (0, long, 4, False), (0, 4097, 0, True), (0, 1, 8, False), (9, 16389, 3, False)]
    for s, d in ((0, 0), (1, 7), (16, 1), (7, 16)):
        run_ranges(emu, inverse, specs, s, d)                             # a workgroup per 32 KB: one a range
        run_ranges(emu, inverse, specs, s, d, hint=4 * 32768)             # four a range, three tiles and a bit to share
    run_ranges(emu, inverse, specs, 1, 7, hint=0)                         # size unknown: the most workgroups a range
    # element sizes that are none of 0, 2, 4, 8 leave their range alone (the last one above), like a skipped one
    run_ranges(emu, inverse, [(0, 100, 1, False), (0, 100, 16, False), (0, 100, 0xFFFFFFFF, False)], 0, 0)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("e", W4.ELEMS)
def test_a_uniform_batch_is_what_the_kernel_of_one_element_size_writes(emu, e, inverse):
    specs = [(0, n, e, n == 255) for n in lengths_for(e)] + [(3, 3 * TILE_BYTES + 5 * e + 1, e, False)]
    for s, d in ((0, 0), (1, 7), (7, 16)):
        for hint in (None, 2 * 32768):
            a = run_ranges(emu, inverse, specs, s, d, hint=hint)
            b = run_ranges(emu, inverse, specs, s, d, hint=hint, call=e)
            assert (a == b).all()


def test_forward_and_inverse_over_a_mixed_batch_are_the_identity(emu):
    sizes = [4097, 300, 3 * TILE_BYTES + 11, 0, 16389, 1]
    elem = np.asarray([4, 0, 8, 2, 2, 4], np.uint32)
    off = np.asarray(np.cumsum([0] + sizes), np.uint64)
    end = int(off[-1])
    data, mid, back = PATTERN[:end].copy(), aligned(end + 32), aligned(end + 32)
    emu.emu_shuffle_ranges(_p(data), _p(off), _p(elem), len(sizes), 0, _p(mid), None, C.c_uint64(max(sizes)))
    emu.emu_shuffle_ranges(_p(mid), _p(off), _p(elem), len(sizes), 1, _p(back), None, C.c_uint64(max(sizes)))
    assert back[:end].tobytes() == data.tobytes() and (back[end:] == GUARD).all() and (mid[end:] == GUARD).all()
    assert mid[:4097].tobytes() == W4.shuffle(data[:4097].tobytes(), 4) and mid[4097:4397].tobytes() == data[4097:4397].tobytes()


# ---------------------------------------------------------------------------------- encode: scan and plan
@pytest.mark.parametrize("store", [False, True])
def test_encode_scan_and_plan_lay_out_a_mixed_batch(emu, store):
    rng = np.random.default_rng(5)
    many = [int(v) for v in rng.integers(0, 9 * BB, 600)]               # more frames than lanes: shares of three
    cases = [(V.LENGTHS, V.ELEMS), (many, [int(v) for v in rng.choice([0, 2, 4, 8], 600)]), ([0, 0, 0], [8, 0, 2]),
             ([4096], [4]), (V.LENGTHS, [0] * V.K), (V.LENGTHS, [8] * V.K)]
    for bits in (12, 13):
        for sizes, elems in cases:
            k = len(sizes)
            in_at, frame_at, base = V.layout(sizes, elems, bits, store)
            c, el = np.asarray(list(sizes) + [G64], np.uint64), np.asarray(list(elems) + [G32], np.uint32)
            a, b, d = np.full(k + 2, G64, np.uint64), np.full(k + 2, G64, np.uint64), np.full(k + 2, G32, np.uint32)
            emu.emu_frames_encode_scan_v4(_p(c), _p(el), k, bits, STORED if store else 0, _p(a), _p(b), _p(d))
            assert a.tolist() == in_at + [G64] and b.tolist() == frame_at + [G64] and d.tolist() == base + [G32]
            total, slab = base[-1], V.sqz_bound(1 << bits)
            in_off, slab_off = np.full(total + 2, G64, np.uint64), np.full(total + 2, G64, np.uint64)
            blk_elem = np.full(total + 1, G32, np.uint32)
            emu.emu_frames_plan_v4(_p(c), _p(el), _p(a), _p(d), k, bits, C.c_uint64(slab), _p(in_off), _p(slab_off),
                                   _p(blk_elem))
            want = [in_at[f] + (j << bits) for f in range(k) for j in range(V.blocks_in(sizes[f], bits))] + [in_at[-1]]
            assert in_off.tolist() == want + [G64]
            assert slab_off.tolist() == [g * slab for g in range(total + 1)] + [G64]
            assert blk_elem.tolist() == [elems[f] for f in range(k) for _ in range(V.blocks_in(sizes[f], bits))] + [G32]
    # the bound of a shuffled frame is the writer's worst case: 8 bytes of record in front of the padding
    assert V.frame_bound(4096, 12, True, 4) == 48 + 4096 and V.frame_bound(4096, 12, True, 0) == 48 + 4096
    assert V.frame_bound(8192, 12, True, 4) == 64 + 8192 and V.frame_bound(8192, 12, True, 0) == 48 + 8192


# ---------------------------------------------------------------------------------- encode: index and seal
def run_index(em, store, fail=None):
    """the mixed batch of frames_v4_cases; fail: (frame, block, errno) -- a block the encoder failed"""
    k, sizes, elems = V.K, V.LENGTHS, V.ELEMS
    in_at, frame_at, base = V.layout(sizes, elems, BITS, store)
    total = base[-1]
    out_bytes = np.asarray([len(s) for f in range(k) for s in V.streams(f)] + [G64], np.uint64)
    crcs = np.asarray([b["content_crc"] for fr in V.frames(False) for b in V.blocks(fr)] + [G32], np.uint32)
    err = np.zeros(total + 1, np.int32)
    if fail is not None:
        err[base[fail[0]] + fail[1]] = fail[2]
    buf = aligned(frame_at[-1] + 64)
    copy_bytes, dense_off = np.full(total + 1, G64, np.uint64), np.full(total + 2, G64, np.uint64)
    dense_rel = np.full(total + k + 1, G64, np.uint64)
    stored = np.full(total + 1, G32, np.uint32)
    fb, st = np.full(k + 1, G64, np.uint64), np.full(k + 1, -7, np.int32)
    em.emu_frames_index_v4(_p(out_bytes), _p(err), _p(crcs), _p(np.asarray(sizes + [G64], np.uint64)),
                           _p(np.asarray(elems + [G32], np.uint32)), _p(np.asarray(frame_at, np.uint64)),
                           _p(np.asarray(base, np.uint32)), k, WB, BITS, STORED if store else 0, _p(buf), _p(copy_bytes),
                           _p(dense_rel), _p(dense_off), _p(stored) if store else None, _p(fb), _p(st))
    assert copy_bytes[total] == G64 and dense_off[total + 1] == G64 and dense_rel[total + k] == G64
    assert stored[total] == G32 and fb[k] == G64 and st[k] == -7
    if not store:
        assert (stored == G32).all()
    return frame_at, base, buf, copy_bytes, dense_off, stored, fb, st


def check_index(store, result, failed=()):
    frame_at, base, buf, copy_bytes, dense_off, stored, fb, st = result
    for f, want in enumerate(V.frames(store)):
        blk = V.blocks(want)
        g0, n = base[f], len(blk)
        slot = buf[frame_at[f]:frame_at[f + 1]]
        assert int(fb[f]) == len(want), f                                   # the size needed is reported either way
        if f in failed:
            assert (slot == GUARD).all() and not copy_bytes[g0:g0 + n].any() and not dense_off[g0:g0 + n].any()
            assert not store or not stored[g0:g0 + n].any()
            continue
        off = V.fields(want)["payload_off"]
        assert want[4] == (4 if V.ELEMS[f] else 2 if store else 1) and int(st[f]) == 0
        assert slot[:off].tobytes() == want[:off], f                        # header, index, record, padding, seal
        assert (slot[off:] == GUARD).all()                                  # the payload is other kernels' business
        assert dense_off[g0:g0 + n].tolist() == [frame_at[f] + b["payload_off"] for b in blk]
        assert copy_bytes[g0:g0 + n].tolist() == [0 if b["stored"] else len(s) for b, s in zip(blk, V.streams(f))]
        if store:
            assert stored[g0:g0 + n].tolist() == [b["stored"] for b in blk]
    last = V.K - 1
    assert int(dense_off[base[-1]]) == (0 if last in failed else frame_at[last] + len(V.frames(store)[last]))
    assert (buf[frame_at[-1]:] == GUARD).all()


@pytest.mark.parametrize("store", [False, True])
def test_index_kernel_writes_the_writers_headers_indexes_records_and_seals(emu, store):
    check_index(store, run_index(emu, store))
    if store:                                                # the noise of frame 7 is stored, shuffled frame or not
        assert all(b["stored"] for b in V.blocks(V.frames(True)[7])) and V.frames(True)[7][4] == 4


@pytest.mark.parametrize("store", [False, True])
def test_a_failed_block_costs_its_frame_alone_shuffled_or_not(emu, store):
    for f, b in ((5, 2), (4, 1), (8, 1), (3, 0)):            # shuffled and plain, in the middle and last; E2BIG is what the
        result = run_index(emu, store, fail=(f, b, errno.E2BIG))         # emit kernel's tree guard answers
        assert int(result[7][f]) == errno.E2BIG
        check_index(store, result, failed=(f,))


# ---------------------------------------------------------------------------------- decode: open
def other_frame():
    """a version-2 frame with another window and 8 KB blocks (a ragged last one)"""
    data = G.content("whole") + G.piece("N")[:1000] + G.piece("b")[:333]
    return data, W2.write_frame(data, 12, 13)


def lay_frames(frames):
    """frames: [(frame bytes, n_blocks, content_bytes, elem)] -> (buffer, items, base): frames at multiples of 16 with
    guard bytes between them, outputs with gaps of 5, 10, ... bytes"""
    k = len(frames)
    items = np.zeros(k + 1, ITEM)
    at, out = 0, 100
    for f, (fr, n, c, e) in enumerate(frames):
        items[f] = (at, len(fr), c, out, n, e)
        at += V.pad16(len(fr)) + 16 * (f % 3)
        out += c + 5 * (f + 1)
    buf = aligned(at + 32)
    for f, (fr, n, c, e) in enumerate(frames):
        a = int(items[f]["frame_at"])
        buf[a:a + len(fr)] = np.frombuffer(fr, np.uint8)
    items[k] = (G64, G64, G64, G64, G32, G32)
    base = np.cumsum([0] + [n for _, n, _, _ in frames]).tolist()
    return buf, items, base


def run_open(em, frames, avail=None):
    k = len(frames)
    buf, items, base = lay_frames(frames)
    if avail is not None:
        items[avail[0]]["avail"] = avail[1]
    got_base = np.full(k + 2, G32, np.uint32)
    em.emu_frames_decode_scan(_p(items), k, _p(got_base))
    assert got_base.tolist() == base + [G32]
    entries = base[-1] + k
    in_off, out_off = np.full(entries + 2, G64, np.uint64), np.full(entries + 2, G64, np.uint64)
    skip, stored = np.full(entries + 1, G32, np.uint32), np.full(entries + 1, G32, np.uint32)
    ent_elem = np.full(entries + 1, G32, np.uint32)
    st = np.full(k + 1, -7, np.int32)
    em.emu_frames_open_v4(_p(buf), _p(items), _p(got_base), k, C.c_uint64(int(items[0]["out_at"])), _p(in_off),
                          _p(out_off), _p(skip), _p(stored), _p(ent_elem), _p(st))
    assert in_off[entries + 1] == G64 and out_off[entries + 1] == G64 and skip[entries] == G32 and stored[entries] == G32
    assert ent_elem[entries] == G32 and st[k] == -7
    return items, base, in_off, out_off, skip, stored, ent_elem, st


def check_open(frames, result, want_status):
    items, base, in_off, out_off, skip, stored, ent_elem, st = result
    for f, (fr, n, c, e) in enumerate(frames):
        e0 = base[f] + f
        at, to = int(items[f]["frame_at"]), int(items[f]["out_at"]) - int(items[0]["out_at"])
        assert int(st[f]) == want_status[f], (f, int(st[f]))
        if want_status[f] != 0:                              # refused: every entry empty and switched off
            ins, outs, sk, sd = [at] * (n + 1), [to] * (n + 1), [1] * (n + 1), [0] * (n + 1)
        else:
            fl, blk = V.fields(fr), V.blocks(fr)
            ins = [at + b["payload_off"] for b in blk] + [at + len(fr)]
            outs = [to + min(j * fl["block_bytes"], fl["content_bytes"]) for j in range(n + 1)]
            sk, sd = [b["stored"] for b in blk] + [1], [b["stored"] for b in blk] + [0]
        assert in_off[e0:e0 + n + 1].tolist() == ins and out_off[e0:e0 + n + 1].tolist() == outs, f
        assert skip[e0:e0 + n + 1].tolist() == sk and stored[e0:e0 + n + 1].tolist() == sd, f
        assert ent_elem[e0:e0 + n + 1].tolist() == [e] * n + [0], f
    end = base[-1] + len(frames)
    assert in_off[end] == in_off[end - 1] and out_off[end] == out_off[end - 1]


def quad(fr, data, e):
    return fr, W.fields(fr)["n_blocks"], len(data), e


def mixed_batch(store):
    return [quad(fr, V.content(f), V.ELEMS[f]) for f, fr in enumerate(V.frames(store))]


@pytest.mark.parametrize("store", [False, True])
def test_open_kernel_lays_out_the_mixed_batch_of_versions_and_element_sizes(emu, store):
    frames = mixed_batch(store)
    d2, f2 = other_frame()
    frames.insert(4, quad(f2, d2, 0))                        # and 8 KB blocks at window 2^12 among them
    assert {fr[4] for fr, _, _, _ in frames} == ({2, 4} if store else {1, 2, 4})
    check_open(frames, run_open(emu, frames), [0] * len(frames))


def test_every_malformed_version_4_variant_costs_its_frame_alone(emu):
    good = mixed_batch(False)
    before, behind = good[6], good[4]                        # a shuffled frame in front, a plain one behind
    data = V.content(5)                                      # three blocks and five bytes, e = 4
    frame = V.frames(False)[5]
    n = W.fields(frame)["n_blocks"]
    variants = [(name, bad, want if head == 0 else errno.EINVAL) for name, bad, head, want in W4.refusals(frame)]
    assert len(variants) == 26
    for name, bad, want in variants:
        frames = [before, (bad, n, len(data), 4), behind]
        check_open(frames, run_open(emu, frames), [0, want, 0])
    for what, mid, want in (
            ("another element size than the record's", (frame, n, len(data), 2), errno.EINVAL),
            ("another element size than the record's", (frame, n, len(data), 8), errno.EINVAL),
            ("a version-4 frame and no element size", (frame, n, len(data), 0), errno.EINVAL),
            ("the table's content is not the header's", (frame, n, len(data) - 1, 4), errno.EINVAL),
            ("the table's blocks are not the header's", (frame, n - 1, len(data), 4), errno.EINVAL)):
        frames = [before, mid, behind]
        check_open(frames, run_open(emu, frames), [0, want, 0])
    frames = [before, (frame, n, len(data), 4), behind]
    check_open(frames, run_open(emu, frames, avail=(1, len(frame) - 8)), [0, errno.E2BIG, 0])
    # a refused first and a refused last frame
    bad = W4.refusals(frame)[0][1]
    frames = [(bad, n, len(data), 4), before, (bad, n, len(data), 4)]
    check_open(frames, run_open(emu, frames), [errno.EINVAL, 0, errno.EINVAL])


def test_an_element_size_for_an_older_frame_and_a_version_3_frame_are_einval_alone(emu):
    good = mixed_batch(True)
    before, behind = good[5], good[6]
    d2, f2 = other_frame()
    plain1 = V.written(V.content(4), 0, False)
    for what, mid in (("version 2 with an element size", quad(f2, d2, 4)),
                      ("version 1 with an element size", quad(plain1, V.content(4), 2)),
                      ("version 3", (G.frame("mixed", 3), V.blocks_in(len(G.content("mixed"))), len(G.content("mixed")), 0)),
                      ("version 3 with an element size",
                       (G.frame("mixed", 3), V.blocks_in(len(G.content("mixed"))), len(G.content("mixed")), 4))):
        frames = [before, mid, behind]
        check_open(frames, run_open(emu, frames), [0, errno.EINVAL, 0])
    # the refusals of the older versions stay what they were, in the middle of a batch with shuffled frames
    for version, R in ((1, W.refusals), (2, W2.refusals)):
        base_frame = V.written(V.content(5), 0, version == 2)
        for name, bad, head, want in R(base_frame):
            size = W.fields(bad)["content_bytes"] if head == 0 else len(V.content(5))
            frames = [before, (bad, V.blocks_in(size), size, 0), behind]
            check_open(frames, run_open(emu, frames), [0, want if head == 0 else errno.EINVAL, 0])
