"""CPU: the call-level rules of the batch calls that know version 4 (include/sqz/sqz.h: sqz_hip_frames_bound_shuf,
sqz_hip_frames_encode_shuf / _decode_shuf and their scratch functions) -- the bound against the sum of the single
bounds, both scratch functions against their formulas as sqz.h writes them, every refusal at the call with the outputs
untouched, a scratch one byte short, ENODEV -- on a machine without a device: the outputs are host arrays between
guard values, which a refused call never follows.  And what the Python calls refuse on the host, and that their
defaults reach the entry points there always were (a recording stand-in for the library, no device)."""
import ctypes as C
import errno

import numpy as np
import pytest

from sqz_amd import _native as N
from test_frames_cpu import (ITEM, M64, Outputs, SIZE_LISTS, _p, bad_tables, blocks_in, frame_bound, pad16, table, u64,
                             up)

E = errno
STORED, SHUFFLE = 1, 4
ELEM_CYCLE = (4, 0, 2, 8, 0)


def u32(values):
    return np.asarray(list(values), np.uint32)


def elems_for(sizes):
    return [ELEM_CYCLE[f % len(ELEM_CYCLE)] for f in range(len(sizes))]


def test_bound_is_the_sum_of_the_single_bounds_each_rounded_up_to_16():
    L = N.lib()
    for bits in (12, 13, 18, 24):
        for store in (False, True):
            for sizes in SIZE_LISTS:
                k = len(sizes)
                for elems in (elems_for(sizes), [0] * k, [8] * k):
                    at = np.full(k + 2, 7, np.uint64)
                    want = [0]
                    for c, e in zip(sizes, elems):
                        one = L.sqz_frame_bound_shuf(c, bits, int(store) | SHUFFLE) if e else \
                            L.sqz_frame_bound_ex(c, bits, int(store))
                        # the record: 8 bytes more in front of the padding
                        assert one == frame_bound(c, bits, store) + (pad16(32 + 8 * blocks_in(c, bits) + 8) -
                                                                     pad16(32 + 8 * blocks_in(c, bits)) if e else 0)
                        want.append(want[-1] + pad16(one))
                    total = L.sqz_hip_frames_bound_shuf(_p(u64(sizes)), _p(u32(elems)), k, bits, int(store), _p(at))
                    assert total == want[-1] and at.tolist() == want + [7]
                    assert L.sqz_hip_frames_bound_shuf(_p(u64(sizes)), _p(u32(elems)), k, bits, int(store), None) == total
                    if not any(elems):
                        assert total == L.sqz_hip_frames_bound(_p(u64(sizes)), k, bits, int(store), None)
    f = L.sqz_hip_frames_bound_shuf
    assert f(None, None, 0, 12, 0, None) == 0                # no frames: no bytes
    for bits in (0, 11, 25):
        assert f(_p(u64([5])), _p(u32([4])), 1, bits, 0, None) == 0
    for flags in (2, 4, 5):                                  # the call's flags are 0 or STORED: the element sizes say the rest
        assert f(_p(u64([5])), _p(u32([4])), 1, 12, flags, None) == 0
    assert f(None, _p(u32([4])), 1, 12, 0, None) == 0 and f(_p(u64([5])), None, 1, 12, 0, None) == 0
    for bad in (1, 3, 5, 6, 16, 0x10004, 0xFFFFFFFF):        # an element size that is none of 0, 2, 4, 8
        assert f(_p(u64([5, 5])), _p(u32([4, bad])), 2, 12, 0, None) == 0
    assert f(_p(u64([M64, 5])), _p(u32([4, 0])), 2, 12, 0, None) == 0                        # sizes that wrap
    assert f(_p(u64([1 << 43])), _p(u32([2])), 1, 12, 1, None) == 0                          # 2^31 blocks


def test_scratch_functions_are_their_formulas():
    L = N.lib()
    f, old = L.sqz_hip_frames_encode_scratch_bytes_shuf, L.sqz_hip_frames_encode_scratch_bytes
    for bits in (12, 13, 18):
        for store in (False, True):
            for sizes in SIZE_LISTS:
                k, T, S = len(sizes), sum(blocks_in(c, bits) for c in sizes), sum(sizes)
                plain = old(_p(u64(sizes)), k, bits, int(store))
                assert f(_p(u64(sizes)), _p(u32([0] * k)), k, bits, int(store)) == plain   # no pass, no scratch for one
                for elems in (elems_for(sizes), [2] * k):
                    assert f(_p(u64(sizes)), _p(u32(elems)), k, bits, int(store)) == \
                        plain + up(4 * k) + up(4 * T + 4) + up(S + 16), (bits, store, sizes)
    assert f(_p(u64([5])), _p(u32([4])), 1, 11, 0) == 0 and f(_p(u64([5])), _p(u32([4])), 1, 12, 4) == 0
    assert f(None, _p(u32([4])), 1, 12, 0) == 0 and f(_p(u64([5])), None, 1, 12, 0) == 0
    assert f(_p(u64([5])), _p(u32([3])), 1, 12, 0) == 0 and f(_p(u64([M64, 5])), _p(u32([4, 4])), 2, 12, 0) == 0
    g, gold = L.sqz_hip_frames_decode_scratch_bytes_shuf, L.sqz_hip_frames_decode_scratch_bytes
    for bits in (12, 13):
        for gap in (0, 5, 4096):
            for sizes in SIZE_LISTS[:7]:
                items = table(sizes, bits, out_gap=gap)
                k, T = len(items), sum(int(i["n_blocks"]) for i in items)
                X = int(items[-1]["out_at"]) + int(items[-1]["content_bytes"]) - int(items[0]["out_at"])
                plain = gold(_p(items), k)
                assert g(_p(items), k) == plain                                          # every last word 0
                named = shuf_table(sizes, elems_for(sizes), bits, out_gap=gap)
                if any(elems_for(sizes)):
                    assert g(_p(named), k) == plain + up(4 * (T + k) + 4) + up(X + 16), (bits, gap, sizes)
                    assert gold(_p(named), k) == 0                                       # the older call: zero != 0
    assert g(None, 1) == 0
    for name, bad, _ in bad_tables():
        if name != "zero_is_not_zero":
            assert g(_p(bad), len(bad)) == 0, name


def shuf_table(sizes, elems, bits=12, out_gap=0):
    """test_frames_cpu.table with the element sizes in the last word and room for the record"""
    items = table(sizes, bits, out_gap)
    at = 0
    for f, (c, e) in enumerate(zip(sizes, elems)):
        room = pad16(frame_bound(c, bits, False)) + 16
        items[f]["frame_at"], items[f]["avail"], items[f]["zero"] = at, room, e
        at += room + 16
    return items


SIZES, ELEMS = [4097, 0, 9000], [4, 0, 2]


def encode_call(L, o, **kw):
    sizes = kw.pop("sizes", SIZES)
    elems = kw.pop("elems", ELEMS)
    a = {"d_in": 0x4000000, "content_bytes": _p(u64(sizes)), "elem_bytes": _p(u32(elems)), "k": len(sizes),
         "win_bits": 15, "block_bits": 12, "flags": 0, "parse": 0, "d_frames": _p(o.frames), "capacity": None,
         "d_frame_bytes": _p(o.frame_bytes), "d_status": _p(o.status), "d_err": _p(o.err), "d_scratch": o.scratch,
         "scratch_bytes": None}
    a.update(kw)
    flags_ok = a["flags"] in (0, 1) and 12 <= a["block_bits"] <= 24
    if a["capacity"] is None:
        a["capacity"] = int(L.sqz_hip_frames_bound_shuf(_p(u64(sizes)), _p(u32(elems)), len(sizes), a["block_bits"],
                                                        a["flags"], None)) if flags_ok else 1 << 20
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = int(L.sqz_hip_frames_encode_scratch_bytes_shuf(
            _p(u64(sizes)), _p(u32(elems)), len(sizes), a["block_bits"], a["flags"])) if flags_ok else 1 << 30
    return L.sqz_hip_frames_encode_shuf(a["d_in"], a["content_bytes"], a["elem_bytes"], a["k"], a["win_bits"],
                                        a["block_bits"], a["flags"], a["parse"], a["d_frames"], a["capacity"],
                                        a["d_frame_bytes"], a["d_status"], a["d_err"], a["d_scratch"],
                                        a["scratch_bytes"], None)


def test_every_refusal_of_an_encode_at_the_call():
    L = N.lib()
    o = Outputs()
    bound = int(L.sqz_hip_frames_bound_shuf(_p(u64(SIZES)), _p(u32(ELEMS)), 3, 12, 0, None))
    need = int(L.sqz_hip_frames_encode_scratch_bytes_shuf(_p(u64(SIZES)), _p(u32(ELEMS)), 3, 12, 0))
    plain_need = int(L.sqz_hip_frames_encode_scratch_bytes(_p(u64(SIZES)), 3, 12, 0))
    assert need > plain_need and bound > int(L.sqz_hip_frames_bound(_p(u64(SIZES)), 3, 12, 0, None))
    refusals = [("flags_2", {"flags": 2}), ("flags_4", {"flags": 4}), ("flags_5", {"flags": 5}),
                ("flags_all_ones", {"flags": 0xFFFFFFFF}),
                ("parse_2", {"parse": 2}), ("parse_all_ones", {"parse": 0xFFFFFFFF}),
                ("win_bits_9", {"win_bits": 9}), ("win_bits_16", {"win_bits": 16}),
                ("block_bits_11", {"block_bits": 11}), ("block_bits_25", {"block_bits": 25}),
                ("capacity_one_short", {"capacity": bound - 1}), ("capacity_0", {"capacity": 0}),
                ("null_sizes", {"content_bytes": None}), ("null_elems", {"elem_bytes": None}),
                ("elem_1", {"elems": [4, 1, 2]}), ("elem_3", {"elems": [3, 0, 0]}), ("elem_16", {"elems": [4, 0, 16]}),
                ("elem_all_ones", {"elems": [0, 0xFFFFFFFF, 0], "capacity": 1 << 20, "scratch_bytes": 1 << 30}),
                ("null_in", {"d_in": None}), ("null_frames", {"d_frames": None}),
                ("misaligned_frames", {"d_frames": o.frames.ctypes.data + 8}),
                ("null_frame_bytes", {"d_frame_bytes": None}), ("null_status", {"d_status": None}),
                ("null_err", {"d_err": None}), ("null_scratch", {"d_scratch": None}),
                ("misaligned_scratch", {"d_scratch": o.scratch + 4}), ("scratch_one_short", {"scratch_bytes": need - 1}),
                ("scratch_of_the_plain_call", {"scratch_bytes": plain_need}),
                ("sizes_wrap", {"sizes": [M64, 5], "elems": [4, 4], "capacity": M64, "scratch_bytes": M64}),
                ("too_many_blocks", {"sizes": [1 << 43], "elems": [2], "capacity": M64, "scratch_bytes": M64})]
    for what, kw in refusals:
        if "elems" in kw and "capacity" not in kw:
            kw = dict(kw, capacity=1 << 20, scratch_bytes=1 << 30)
        assert encode_call(L, o, **kw) == E.EINVAL, what
        assert o.untouched(), what
    # all element sizes 0: the plain call's scratch is enough, and one byte less is not
    assert encode_call(L, o, elems=[0, 0, 0], scratch_bytes=plain_need - 1) == E.EINVAL and o.untouched()
    # no frames: nothing to do, whatever the pointers are -- but the parameters are still checked
    assert encode_call(L, o, sizes=[], elems=[], d_in=None, content_bytes=None, elem_bytes=None, d_frames=None,
                       d_scratch=None, capacity=0, scratch_bytes=0) == 0
    assert encode_call(L, o, sizes=[], elems=[], flags=2) == E.EINVAL
    assert encode_call(L, o, sizes=[], elems=[], parse=7) == E.EINVAL
    assert o.untouched()


def decode_call(L, o, items, **kw):
    a = {"d_frames": _p(o.frames), "table": _p(items), "k": len(items), "d_out": 0x4000000, "d_err": _p(o.err),
         "d_status": _p(o.status), "d_scratch": o.scratch, "scratch_bytes": None}
    a.update(kw)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = int(L.sqz_hip_frames_decode_scratch_bytes_shuf(_p(items), len(items))) or 1 << 40
    return L.sqz_hip_frames_decode_shuf(a["d_frames"], a["table"], a["k"], a["d_out"], a["d_err"], a["d_status"],
                                        a["d_scratch"], a["scratch_bytes"], None)


def test_every_refusal_of_a_decode_at_the_call():
    L = N.lib()
    o = Outputs()
    good = shuf_table(SIZES, ELEMS)
    need = int(L.sqz_hip_frames_decode_scratch_bytes_shuf(_p(good), 3))
    plain_need = int(L.sqz_hip_frames_decode_scratch_bytes(_p(table(SIZES)), 3))
    assert need > plain_need
    for what, bad, want in bad_tables():                     # the plain table's, with "zero" now an element size: 1 is none
        assert decode_call(L, o, bad) == want, what
        assert o.untouched(), what
    for bad_elem in (1, 3, 5, 6, 16, 0x10004, 0xFFFFFFFF):
        t = good.copy()
        t[1]["zero"] = bad_elem
        assert decode_call(L, o, t, scratch_bytes=1 << 40) == E.EINVAL and o.untouched()
    for what, kw in (("null_items", {"table": None}), ("null_frames", {"d_frames": None}),
                     ("misaligned_frames", {"d_frames": o.frames.ctypes.data + 8}), ("null_out", {"d_out": None}),
                     ("null_err", {"d_err": None}), ("null_status", {"d_status": None}),
                     ("null_scratch", {"d_scratch": None}), ("misaligned_scratch", {"d_scratch": o.scratch + 8}),
                     ("scratch_one_short", {"scratch_bytes": need - 1}),
                     ("scratch_of_the_plain_call", {"scratch_bytes": plain_need})):
        assert decode_call(L, o, good, **kw) == E.EINVAL, what
        assert o.untouched(), what
    assert decode_call(L, o, table(SIZES), scratch_bytes=plain_need - 1) == E.EINVAL and o.untouched()
    # header, index and -- where an element size is named -- the record outside avail: E2BIG, as for the single call
    for f in range(3):
        short = good.copy()
        short[f]["avail"] = 32 + 8 * int(short[f]["n_blocks"]) + (8 if ELEMS[f] else 0) - 1
        assert decode_call(L, o, short) == E.E2BIG and o.untouched()
    assert L.sqz_hip_frames_decode_shuf(None, None, 0, None, None, None, None, 0, None) == 0  # no frames


def test_enodev_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    L = N.lib()
    o = Outputs()
    assert encode_call(L, o) == E.ENODEV and encode_call(L, o, flags=1, parse=1, win_bits=10, block_bits=24) == E.ENODEV
    assert encode_call(L, o, elems=[0, 0, 0]) == E.ENODEV and encode_call(L, o, elems=[8, 8, 8]) == E.ENODEV
    assert encode_call(L, o, sizes=[0, 0], elems=[2, 0], d_in=None, d_err=None) == E.ENODEV   # empty contents
    assert decode_call(L, o, shuf_table(SIZES, ELEMS)) == E.ENODEV
    assert decode_call(L, o, table(SIZES)) == E.ENODEV
    assert decode_call(L, o, shuf_table([0, 0], [4, 0]), d_out=None, d_err=None) == E.ENODEV
    exact = shuf_table(SIZES, ELEMS)                                                 # avail that just covers the record
    exact[0]["avail"] = 32 + 8 * int(exact[0]["n_blocks"]) + 8
    assert decode_call(L, o, exact) == E.ENODEV
    d = np.zeros(64, np.uint8)
    assert L.sqz_hip_shuffle_ranges(_p(d), _p(u64([0, 8])), _p(u32([4])), 1, 0, _p(d[32:]), None, None) == E.ENODEV
    assert L.sqz_hip_shuffle_ranges(_p(d), _p(u64([0, 8])), None, 1, 0, _p(d[32:]), None, None) == E.EINVAL
    assert L.sqz_hip_shuffle_ranges(_p(d), _p(u64([0, 8])), _p(u32([4])), 1, 0, _p(d), None, None) == E.EINVAL
    assert L.sqz_hip_shuffle_ranges(None, None, None, 0, 0, None, None, None) == 0
    assert o.untouched()


# ---------------------------------------------------------------------------------- Python
def test_the_python_calls_refuse_a_bad_shuffle_before_anything_native_runs(monkeypatch):
    import torch
    from sqz_amd import frame as F

    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(F.N, "lib", no_library)
    d = torch.zeros(64, dtype=torch.uint8)
    bad = (True, False, 1, 3, 16, -2, 4.0, "4", b"\x04", [4], [4, 0, 2], [4, 3], [4, True], [4, 2.0], [4, None],
           (8, "2"), object())
    for shuffle in bad:
        with pytest.raises(ValueError, match="shuffle|element size"):
            F.frames_bound([8, 8], shuffle=shuffle)
        with pytest.raises(ValueError, match="shuffle|element size"):
            F.encode_frames(d, [8, 8], shuffle=shuffle)
        with pytest.raises(ValueError, match="shuffle|element size"):
            F.compress_frames([b"abc", b"def"], shuffle=shuffle)


class Recorder:
    """stands in for the library object: records the entry points asked for, answers every call with 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            if name.startswith("sqz_hip_frames_bound"):
                at = args[-1]
                for j in range(len(at)):
                    at[j] = 64 * j
                return 64 * (len(at) - 1)
            return 256 if "scratch_bytes" in name else 0
        return call


@pytest.fixture
def recorded(monkeypatch):
    import torch
    from sqz_amd import frame as F
    rec = Recorder()
    monkeypatch.setattr(F.N, "lib", lambda: rec)
    monkeypatch.setattr(F, "_stream", lambda: None)
    monkeypatch.setattr(F, "_pinned", lambda array: torch.zeros(8, dtype=torch.uint8))
    monkeypatch.setattr(F, "_scratch_for", lambda device, need: torch.zeros(max(need, 16), dtype=torch.uint8))
    return F, rec


def test_the_defaults_reach_the_entry_points_there_always_were(recorded):
    import torch
    F, rec = recorded
    d_in, d_out = torch.zeros(64, dtype=torch.uint8), torch.zeros(256, dtype=torch.uint8)
    for shuffle in (None, 0):
        rec.calls.clear()
        F.frames_bound([8, 8], 12, shuffle=shuffle)
        F.encode_frames(d_in, [8, 8], 15, 12, d_out=d_out, shuffle=shuffle)
        assert rec.calls == ["sqz_hip_frames_bound", "sqz_hip_frames_bound", "sqz_hip_frames_encode_scratch_bytes",
                             "sqz_hip_frames_encode"]
    rec.calls.clear()
    F.frames_bound([8, 8], 12)
    F.encode_frames(d_in, [8, 8], 15, 12, d_out=d_out)
    assert rec.calls == ["sqz_hip_frames_bound", "sqz_hip_frames_bound", "sqz_hip_frames_encode_scratch_bytes",
                         "sqz_hip_frames_encode"]
    for shuffle in (4, [4, 0], (0, 0), np.asarray([2, 8]).tolist()):
        rec.calls.clear()
        F.frames_bound([8, 8], 12, shuffle=shuffle)
        F.encode_frames(d_in, [8, 8], 15, 12, d_out=d_out, shuffle=shuffle)
        assert rec.calls == ["sqz_hip_frames_bound_shuf", "sqz_hip_frames_bound_shuf",
                             "sqz_hip_frames_encode_scratch_bytes_shuf", "sqz_hip_frames_encode_shuf"]
    infos = [{"n_blocks": 1, "content_bytes": 8, "version": 1}, {"n_blocks": 1, "content_bytes": 8, "version": 4,
                                                                 "elem_bytes": 4}]
    d_frames = torch.zeros(256, dtype=torch.uint8)
    rec.calls.clear()
    F.decode_frames(d_frames, [0, 64], infos=infos, d_out=d_out)
    F.decode_frames(d_frames, [0, 64], infos=infos, d_out=d_out, shuffled=False)
    assert rec.calls == ["sqz_hip_frames_decode_scratch_bytes", "sqz_hip_frames_decode"] * 2
    rec.calls.clear()
    F.decode_frames(d_frames, [0, 64], infos=infos, d_out=d_out, shuffled=True)
    assert rec.calls == ["sqz_hip_frames_decode_scratch_bytes_shuf", "sqz_hip_frames_decode_shuf"]


def test_the_table_of_a_shuffled_decode_carries_the_element_sizes(recorded, monkeypatch):
    import torch
    F, rec = recorded
    tables = []
    monkeypatch.setattr(F, "_pinned", lambda array: tables.append(np.array(array)) or torch.zeros(8, dtype=torch.uint8))
    infos = [{"n_blocks": 1, "content_bytes": 8, "version": 4, "elem_bytes": 8},
             {"n_blocks": 2, "content_bytes": 5000, "version": 2},
             {"n_blocks": 1, "content_bytes": 9, "version": 4, "elem_bytes": 2},
             {"n_blocks": 1, "content_bytes": 9, "version": 4}]           # a header alone: no element size in reach
    d_frames, d_out = torch.zeros(8192, dtype=torch.uint8), torch.zeros(8192, dtype=torch.uint8)
    F.decode_frames(d_frames, [0, 64, 6000, 6096], infos=infos, d_out=d_out, shuffled=True)
    assert tables[-1]["zero"].tolist() == [8, 0, 2, 0] and tables[-1].dtype.itemsize == 40
    F.decode_frames(d_frames, [0, 64, 6000, 6096], infos=infos, d_out=d_out)
    assert tables[-1]["zero"].tolist() == [0, 0, 0, 0]


def test_the_exports():
    L = N.lib()
    for name in ("sqz_hip_frames_bound_shuf", "sqz_hip_frames_encode_scratch_bytes_shuf", "sqz_hip_frames_encode_shuf",
                 "sqz_hip_frames_decode_scratch_bytes_shuf", "sqz_hip_frames_decode_shuf", "sqz_hip_shuffle_ranges"):
        assert name in N.PROTOTYPES and getattr(L, name) is not None
    assert C.sizeof(N.FramesItem) == 40 == ITEM.itemsize
