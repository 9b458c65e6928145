"""CPU: the call-level rules of sqz_hip_frames_encode / _decode (include/sqz/sqz.h) -- the bound and both scratch
functions against their formulas written out here, every refusal at the call with the outputs untouched, ENODEV -- on a
machine without a device: the outputs are host arrays between guard values, which a refused call never follows.  And
what the Python calls refuse on the host, and the exports."""
import ctypes as C
import errno

import numpy as np
import pytest

from sqz_amd import _native as N

E = errno
M64 = (1 << 64) - 1
STORED = 1
ITEM = np.dtype([("frame_at", "<u8"), ("avail", "<u8"), ("content_bytes", "<u8"), ("out_at", "<u8"),
                 ("n_blocks", "<u4"), ("zero", "<u4")])


def up(v):
    return (v + 255) & ~255


def pad16(v):
    return (v + 15) & ~15


def blocks_in(c, bits):
    return (c + (1 << bits) - 1) >> bits


def sqz_bound(n):
    return (2 * n + 1024 + 7) & ~7


def frame_bound(c, bits, store):
    bb = 1 << bits
    off = pad16(32 + 8 * blocks_in(c, bits))
    if store:
        return off + ((c + 7) & ~7)
    return off + (c // bb) * sqz_bound(bb) + (sqz_bound(c % bb) if c % bb else 0)


def encode_scratch_formula(sizes, bits, store):
    k, T, S = len(sizes), sum(blocks_in(c, bits) for c in sizes), sum(sizes)
    tables = up(8 * k) + 2 * up(8 * (k + 1)) + up(4 * (k + 1))
    lists = 2 * up(8 * (T + 1)) + up(4 * T + 4) + 2 * up(8 * T)
    dense = up(8 * (T + k)) + up(8 * (T + 1)) + (up(4 * T + 4) if store else 0)
    codec = up(4 * T) + 2 * (S + 64) * 4                               # sqz_hip_encode_scratch_bytes(T, S)
    return tables + lists + dense + up(T * sqz_bound(1 << bits)) + up(codec)


def decode_scratch_formula(items):
    k, T = len(items), sum(int(i["n_blocks"]) for i in items)
    Et = T + k
    X = int(items[-1]["out_at"]) + int(items[-1]["content_bytes"]) - int(items[0]["out_at"])
    codec = up(4 * Et) + (X + 64) * 4                                  # sqz_hip_decode_scratch_bytes(E, X)
    return up(40 * k) + up(4 * (k + 1)) + 2 * up(8 * (Et + 1)) + 4 * up(4 * Et + 4) + up(codec)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def u64(values):
    return np.asarray(list(values), np.uint64)


SIZE_LISTS = [[0], [1], [4096], [4097], [0, 1, 4096, 4097, 3 * 4096 + 5, 70 * 4096, 300 * 4096 - 1], [5] * 70,
              [1 << 20] * 64, [0, 0, 0], [(1 << 24) + 1, 7]]


def test_bound_is_the_sum_of_the_frames_bounds_each_rounded_up_to_16():
    L = N.lib()
    assert L.sqz_frame_bound_ex(4097, 12, 0) == frame_bound(4097, 12, False)
    assert L.sqz_frame_bound_ex(4097, 12, STORED) == frame_bound(4097, 12, True)
    for bits in (12, 13, 18, 24):
        for store in (False, True):
            for sizes in SIZE_LISTS:
                k = len(sizes)
                at = np.full(k + 2, 7, np.uint64)
                want = [0]
                for c in sizes:
                    assert L.sqz_frame_bound_ex(c, bits, int(store)) == frame_bound(c, bits, store)
                    want.append(want[-1] + pad16(frame_bound(c, bits, store)))
                total = L.sqz_hip_frames_bound(_p(u64(sizes)), k, bits, int(store), _p(at))
                assert total == want[-1] and at.tolist() == want + [7]
                assert L.sqz_hip_frames_bound(_p(u64(sizes)), k, bits, int(store), None) == total
    assert L.sqz_hip_frames_bound(None, 0, 12, 0, None) == 0             # no frames: no bytes
    for bits in (0, 11, 25):
        assert L.sqz_hip_frames_bound(_p(u64([5])), 1, bits, 0, None) == 0
    assert L.sqz_hip_frames_bound(_p(u64([5])), 1, 12, 2, None) == 0
    assert L.sqz_hip_frames_bound(None, 1, 12, 0, None) == 0
    assert L.sqz_hip_frames_bound(_p(u64([M64, 5])), 2, 12, 0, None) == 0                    # sizes that wrap
    assert L.sqz_hip_frames_bound(_p(u64([1 << 61, 1 << 61, 1 << 61, 1 << 61])), 4, 24, 1, None) == 0
    assert L.sqz_hip_frames_bound(_p(u64([1 << 43])), 1, 12, 1, None) == 0                   # 2^31 blocks


def test_scratch_functions_are_their_formulas():
    L = N.lib()
    f = L.sqz_hip_frames_encode_scratch_bytes
    assert L.sqz_bound(4096) == sqz_bound(4096)
    assert L.sqz_hip_encode_scratch_bytes(3, 9000) == up(12) + 2 * (9000 + 64) * 4
    assert L.sqz_hip_decode_scratch_bytes(5, 9000) == up(20) + (9000 + 64) * 4
    for bits in (12, 13, 18):
        for store in (False, True):
            for sizes in SIZE_LISTS:
                assert f(_p(u64(sizes)), len(sizes), bits, int(store)) == encode_scratch_formula(sizes, bits, store)
    assert f(_p(u64([5])), 1, 11, 0) == 0 and f(_p(u64([5])), 1, 12, 4) == 0 and f(None, 1, 12, 0) == 0
    assert f(_p(u64([M64, 5])), 2, 12, 0) == 0
    g = L.sqz_hip_frames_decode_scratch_bytes
    for bits in (12, 13):
        for gap in (0, 5, 4096):
            for sizes in SIZE_LISTS[:7]:
                items = table(sizes, bits, out_gap=gap)
                assert g(_p(items), len(items)) == decode_scratch_formula(items), (bits, gap, sizes)
    assert g(None, 1) == 0
    for bad in bad_tables():
        assert g(_p(bad[1]), len(bad[1])) == 0, bad[0]


def table(sizes, bits=12, out_gap=0, out_base=64):
    """a table the call takes: frames of their worst-case size 16 bytes apart, outputs out_gap bytes apart"""
    items = np.zeros(len(sizes), ITEM)
    at, out = 0, out_base
    for f, c in enumerate(sizes):
        room = pad16(frame_bound(c, bits, False))
        items[f] = (at, room, c, out, blocks_in(c, bits), 0)
        at += room + 16
        out += c + out_gap
    return items


def bad_tables():
    """(name, table, errno): each the good table of three frames with ONE change"""
    good = table([4097, 0, 9000])
    out = []

    def put(name, f, field, value, want=E.EINVAL):
        t = good.copy()
        t[f][field] = value
        out.append((name, t, want))

    put("frame_at_not_a_multiple_of_16", 1, "frame_at", int(good[1]["frame_at"]) + 8)
    put("zero_is_not_zero", 2, "zero", 1)
    put("frames_overlap", 0, "avail", int(good[1]["frame_at"]) + 1)
    put("frames_descend", 2, "frame_at", 0)
    put("outputs_overlap", 0, "content_bytes", int(good[1]["out_at"]) - int(good[0]["out_at"]) + 1)
    put("outputs_descend", 2, "out_at", 0)
    put("frame_end_wraps", 2, "avail", M64)
    put("output_end_wraps", 2, "out_at", M64 - 10)
    put("too_many_blocks", 1, "n_blocks", 0x7FFFFFFF)
    return out


class Outputs:
    """host arrays in the outputs' places, between guard values"""

    def __init__(self):
        self.frames = np.full(1 << 16, 0xA5, np.uint8)
        self.frames = self.frames[(-self.frames.ctypes.data) % 16:][:1 << 15]
        self.frame_bytes = np.full(16, 0x77, np.uint64)
        self.status = np.full(16, -7, np.int32)
        self.err = np.full(64, -7, np.int32)
        self.scratch = 0x10000000

    def untouched(self):
        return (self.frames == 0xA5).all() and (self.frame_bytes == 0x77).all() and (self.status == -7).all() and \
               (self.err == -7).all()


def encode_call(L, o, **kw):
    sizes = kw.pop("sizes", [4097, 0, 9000])
    a = {"d_in": 0x4000000, "content_bytes": _p(u64(sizes)), "k": len(sizes), "win_bits": 15, "block_bits": 12,
         "flags": 0, "parse": 0, "d_frames": _p(o.frames), "capacity": None, "d_frame_bytes": _p(o.frame_bytes),
         "d_status": _p(o.status), "d_err": _p(o.err), "d_scratch": o.scratch, "scratch_bytes": None}
    a.update(kw)
    flags_ok = a["flags"] in (0, 1) and 12 <= a["block_bits"] <= 24
    if a["capacity"] is None:
        a["capacity"] = int(L.sqz_hip_frames_bound(_p(u64(sizes)), len(sizes), a["block_bits"], a["flags"], None)) \
            if flags_ok else 1 << 20
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = int(L.sqz_hip_frames_encode_scratch_bytes(_p(u64(sizes)), len(sizes), a["block_bits"],
                                                                       a["flags"])) if flags_ok else 1 << 30
    return L.sqz_hip_frames_encode(a["d_in"], a["content_bytes"], a["k"], a["win_bits"], a["block_bits"], a["flags"],
                                   a["parse"], a["d_frames"], a["capacity"], a["d_frame_bytes"], a["d_status"],
                                   a["d_err"], a["d_scratch"], a["scratch_bytes"], None)


def test_every_refusal_of_an_encode_at_the_call():
    L = N.lib()
    o = Outputs()
    bound = int(L.sqz_hip_frames_bound(_p(u64([4097, 0, 9000])), 3, 12, 0, None))
    need = int(L.sqz_hip_frames_encode_scratch_bytes(_p(u64([4097, 0, 9000])), 3, 12, 0))
    refusals = [("flags_2", {"flags": 2}), ("flags_3", {"flags": 3}), ("flags_all_ones", {"flags": 0xFFFFFFFF}),
                ("parse_2", {"parse": 2}), ("parse_all_ones", {"parse": 0xFFFFFFFF}),
                ("win_bits_9", {"win_bits": 9}), ("win_bits_16", {"win_bits": 16}),
                ("block_bits_11", {"block_bits": 11}), ("block_bits_25", {"block_bits": 25}),
                ("capacity_one_short", {"capacity": bound - 1}), ("capacity_0", {"capacity": 0}),
                ("null_sizes", {"content_bytes": None}), ("null_in", {"d_in": None}), ("null_frames", {"d_frames": None}),
                ("misaligned_frames", {"d_frames": o.frames.ctypes.data + 8}),
                ("null_frame_bytes", {"d_frame_bytes": None}), ("null_status", {"d_status": None}),
                ("null_err", {"d_err": None}), ("null_scratch", {"d_scratch": None}),
                ("misaligned_scratch", {"d_scratch": o.scratch + 4}), ("scratch_one_short", {"scratch_bytes": need - 1}),
                ("sizes_wrap", {"sizes": [M64, 5], "capacity": M64, "scratch_bytes": M64}),
                ("too_many_blocks", {"sizes": [1 << 43], "capacity": M64, "scratch_bytes": M64})]
    for what, kw in refusals:
        assert encode_call(L, o, **kw) == E.EINVAL, what
        assert o.untouched(), what
    # no frames: nothing to do, whatever the pointers are -- but the parameters are still checked
    assert encode_call(L, o, sizes=[], d_in=None, content_bytes=None, d_frames=None, d_scratch=None, capacity=0,
                       scratch_bytes=0) == 0
    assert encode_call(L, o, sizes=[], flags=2) == E.EINVAL and encode_call(L, o, sizes=[], parse=7) == E.EINVAL
    assert o.untouched()


def decode_call(L, o, items, **kw):
    a = {"d_frames": _p(o.frames), "table": _p(items), "k": len(items), "d_out": 0x4000000, "d_err": _p(o.err),
         "d_status": _p(o.status), "d_scratch": o.scratch, "scratch_bytes": None}
    a.update(kw)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = int(L.sqz_hip_frames_decode_scratch_bytes(_p(items), len(items))) or 1 << 40
    return L.sqz_hip_frames_decode(a["d_frames"], a["table"], a["k"], a["d_out"], a["d_err"], a["d_status"],
                                   a["d_scratch"], a["scratch_bytes"], None)


def test_every_refusal_of_a_decode_at_the_call():
    L = N.lib()
    o = Outputs()
    good = table([4097, 0, 9000])
    need = int(L.sqz_hip_frames_decode_scratch_bytes(_p(good), 3))
    for what, bad, want in bad_tables():
        assert decode_call(L, o, bad) == want, what
        assert o.untouched(), what
    for what, kw in (("null_items", {"table": None}), ("null_frames", {"d_frames": None}),
                     ("misaligned_frames", {"d_frames": o.frames.ctypes.data + 8}), ("null_out", {"d_out": None}),
                     ("null_err", {"d_err": None}), ("null_status", {"d_status": None}),
                     ("null_scratch", {"d_scratch": None}), ("misaligned_scratch", {"d_scratch": o.scratch + 8}),
                     ("scratch_one_short", {"scratch_bytes": need - 1})):
        assert decode_call(L, o, good, **kw) == E.EINVAL, what
        assert o.untouched(), what
    # header and index outside avail: E2BIG, as for the single call
    for f in range(3):
        short = good.copy()
        short[f]["avail"] = 32 + 8 * int(short[f]["n_blocks"]) - 1
        assert decode_call(L, o, short) == E.E2BIG and o.untouched()
    assert L.sqz_hip_frames_decode(None, None, 0, None, None, None, None, 0, None) == 0      # no frames


def test_enodev_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    L = N.lib()
    o = Outputs()
    assert encode_call(L, o) == E.ENODEV and encode_call(L, o, flags=1, parse=1, win_bits=10, block_bits=24) == E.ENODEV
    assert encode_call(L, o, sizes=[0, 0], d_in=None, d_err=None) == E.ENODEV          # empty contents: 32-byte frames
    assert decode_call(L, o, table([4097, 0, 9000])) == E.ENODEV
    assert decode_call(L, o, table([0, 0]), d_out=None, d_err=None) == E.ENODEV
    touching = table([4096, 4096])                                                   # neighbours are not overlaps
    touching[0]["avail"] = int(touching[1]["frame_at"])
    assert decode_call(L, o, touching) == E.ENODEV
    assert o.untouched()


def test_the_python_calls_refuse_on_the_host():
    import torch
    from sqz_amd import frame as F
    d = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="parse"):
        F.encode_frames(d, [8, 8], parse="eager")
    with pytest.raises(ValueError, match="parse"):
        F.compress_frames([b"abc"], parse="eager")
    for bits in (11, 25, True, 12.0):
        with pytest.raises(ValueError, match="block_bits"):
            F.encode_frames(d, [8, 8], block_bits=bits)
        with pytest.raises(ValueError, match="block_bits"):
            F.frames_bound([8, 8], block_bits=bits)
        with pytest.raises(ValueError, match="block_bits"):
            F.compress_frames([b"abc"], block_bits=bits)
    for bits in (9, 16):
        with pytest.raises(ValueError, match="win_bits"):
            F.encode_frames(d, [8, 8], win_bits=bits)
    with pytest.raises(ValueError, match="sizes"):
        F.encode_frames(d, [8, -1])
    with pytest.raises(ValueError, match="d_in"):
        F.encode_frames(d, [60, 8])
    info = {"n_blocks": 1, "content_bytes": 8}
    with pytest.raises(ValueError, match="multiple of 16"):
        F.decode_frames(d, [0, 40], infos=[info, info])
    with pytest.raises(ValueError, match="infos"):
        F.decode_frames(d, [0, 48], infos=[info])
    with pytest.raises(ValueError, match="out_at"):
        F.decode_frames(d, [0, 48], infos=[info, info], out_at=[0])
    with pytest.raises(ValueError, match="ascending"):
        F.decode_frames(d, [48, 0], infos=[info, info])
    with pytest.raises(ValueError, match="ascending"):
        F.decode_frames(d, [0, 64], infos=[info, info])


def test_frames_bound_in_python_and_the_exports():
    import sqz_amd
    from sqz_amd import frame as F
    total, at = F.frames_bound([4097, 0, 9000], 12, store=True)
    assert at == [0, pad16(frame_bound(4097, 12, True)), pad16(frame_bound(4097, 12, True)) + 32]
    assert total == at[2] + pad16(frame_bound(9000, 12, True))
    assert F.frames_bound([]) == (0, [])
    for name in ("frames_bound", "encode_frames", "decode_frames", "compress_frames", "decompress_frames"):
        assert name in sqz_amd.__all__ and name in sqz_amd._FRAME and getattr(sqz_amd, name) is getattr(F, name)
    assert C.sizeof(N.FramesItem) == 40 == ITEM.itemsize
