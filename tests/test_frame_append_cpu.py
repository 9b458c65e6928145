"""CPU: the call-level rules of sqz_hip_frame_append / _append_dict (include/sqz/sqz.h) -- the scratch function against
a restatement of its formula, every refusal at the call, ENODEV -- on a machine without a device.  The pointers are
never followed here.  And what append_frame refuses on the host, before anything is enqueued."""
import errno

import pytest

from sqz_amd import _native as N

E = errno
M64 = (1 << 64) - 1


def up(v):
    return (v + 255) & ~255


def shape(n, C, A, bits):
    """(t counted, m) by the header's arithmetic"""
    t = C % (1 << bits)
    head = t if n > 0 and t > 0 and A > 0 else 0
    m = (head + A + (1 << bits) - 1) >> bits if A > 0 else 0
    return head, m


def scratch_formula(n, C, A, bits, D):
    """the header's terms, one by one"""
    w = (n + 31) // 32
    head, m = shape(n, C, A, bits)
    open_one = 2 * up(4 * w + 4) + 256 + up(8) + 2 * up(24) + 4 * up(12)
    staging = up((head + A if A > 0 else 0) + 16)
    lists = 2 * up(8 * (m + 1)) + up(8 * m + 8) + 2 * up(4 * m + 4)
    table = up(8 * (m + 2)) + 2 * up(8 * (m + 1)) + 256
    dict_index = 256 + 2 * up(4 * (D + 64)) if D > 0 else 0
    slabs = up(m * (2 * (1 << bits) + 1024))                         # m * sqz_bound(2^bits)
    decode = up(2 * 4) + ((1 << bits) + 64) * 4                      # sqz_hip_decode_scratch_bytes(2, 2^bits)
    encode = up(m * 4) + 2 * ((m << bits) + 64) * 4                  # sqz_hip_encode_scratch_bytes(m, m << bits)
    return open_one + staging + lists + table + dict_index + slabs + up(max(decode, encode))


def test_scratch_function_is_its_formula_monotone_and_zero_for_bad_arguments():
    L = N.lib()
    f = L.sqz_hip_frame_append_scratch_bytes
    for bits in (12, 13, 18, 24):
        bb = 1 << bits
        for n, t in ((0, 0), (1, 0), (1, 1), (31, 904), (32, 0), (33, bb - 1), (300, 904), (16384, 100)):
            C = n * bb if t == 0 else (n - 1) * bb + t
            for A in (0, 1, bb - t - 1, bb - t, bb - t + 1, 3 * bb + 1, 1 << 26):
                for D in (0, 1, 3000, 32767):
                    assert f(n, C, A, bits, D) == scratch_formula(n, C, A, bits, D), (n, C, A, bits, D)
    assert L.sqz_bound(4096) == 2 * 4096 + 1024
    assert L.sqz_hip_decode_scratch_bytes(2, 4096) == up(8) + (4096 + 64) * 4
    assert L.sqz_hip_encode_scratch_bytes(3, 3 << 12) == up(12) + 2 * ((3 << 12) + 64) * 4
    # monotone in the blocks, the data, the block size and the dictionary (the content goes with the blocks)
    base = (300, 299 * 4096 + 904, 5000, 12, 100)
    for step in (1, 7, 1000):
        assert f(300 + step, (299 + step) * 4096 + 904, 5000, 12, 100) >= f(*base), step
        assert f(300, 299 * 4096 + 904, 5000 + step, 12, 100) >= f(*base), step
        assert f(300, 299 * 4096 + 904, 5000, 12, 100 + step) >= f(*base), step
    for more in (1, 7, 12):
        assert f(300, 299 * 4096 + 904, 5000, 12 + more, 100) >= f(*base), more
    # a ragged last block costs its bytes in the staging area and never a block less to encode
    assert f(300, 299 * 4096 + 904, 5000, 12, 0) >= f(300, 300 * 4096, 5000, 12, 0)
    # about 11 bytes per byte of data for a long append: 1 staged, 2 of slab, 8 of the encoder's
    long = f(16384, 16384 * 4096, 1 << 30, 12, 0)
    assert 10.5 * (1 << 30) < long < 11.5 * (1 << 30)
    for bits in (0, 11, 25, 64):
        assert f(300, 299 * 4096 + 904, 5000, bits, 0) == 0
    assert f(300, 299 * 4096 + 904, 5000, 12, 32768) == 0
    # sizes that wrap, and more new blocks than 32 bits count
    assert f(300, 299 * 4096 + 904, M64, 12, 0) == 0 and f(300, 299 * 4096 + 904, M64 - 299 * 4096 - 903, 12, 0) == 0
    assert f(300, 299 * 4096 + 904, 1 << 44, 12, 0) == 0


def _args(L, **kw):
    """a call that passes every check at the call (on made-up device pointers, which nothing follows)"""
    a = {"d_frame": 0x10000, "avail": 0x1000, "n_blocks": 3, "content_bytes": 9096, "win_bits": 15, "block_bits": 12,
         "d_data": 0x40000, "data_bytes": 400, "parse": 0, "d_dict": 0x9000, "dict_bytes": 3000,
         "d_new_frame": 0x100000, "capacity": 0x8000, "d_frame_bytes": 0x5800, "d_blocks_encoded": 0x7000,
         "d_status": 0x8000, "d_scratch": 0x1000000, "scratch_bytes": None, "dict": False}
    a.update(kw)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = int(L.sqz_hip_frame_append_scratch_bytes(a["n_blocks"], a["content_bytes"], a["data_bytes"], 12,
                                                                      a["dict_bytes"] if a["dict"] else 0))
    return a


def call(L, dict_flavour, **kw):
    a = _args(L, dict=dict_flavour, **kw)
    head = (a["d_frame"], a["avail"], a["n_blocks"], a["content_bytes"], a["win_bits"], a["block_bits"], a["d_data"],
            a["data_bytes"], a["parse"])
    tail = (a["d_new_frame"], a["capacity"], a["d_frame_bytes"], a["d_blocks_encoded"], a["d_status"], a["d_scratch"],
            a["scratch_bytes"], None)
    if dict_flavour:
        return L.sqz_hip_frame_append_dict(*head, a["d_dict"], a["dict_bytes"], *tail)
    return L.sqz_hip_frame_append(*head, *tail)


BIG = 1 << 40                                # a scratch size for the arguments whose own the function answers 0 for
REFUSALS = [("block_bits_11", {"block_bits": 11}), ("block_bits_25", {"block_bits": 25}),
            ("win_bits_9", {"win_bits": 9}), ("win_bits_16", {"win_bits": 16}),
            ("n_blocks_is_not_the_contents", {"n_blocks": 4}), ("content_is_not_n_blocks", {"content_bytes": 3 * 4096 + 1}),
            ("null_frame", {"d_frame": None}), ("misaligned_frame", {"d_frame": 0x10008}),
            ("null_scratch", {"d_scratch": None}), ("misaligned_scratch", {"d_scratch": 0x1000004}),
            ("null_status", {"d_status": None}), ("null_blocks_encoded", {"d_blocks_encoded": None}),
            ("null_data", {"d_data": None}), ("null_new_frame", {"d_new_frame": None}),
            ("misaligned_new_frame", {"d_new_frame": 0x100008}), ("null_frame_bytes", {"d_frame_bytes": None}),
            ("parse_2", {"parse": 2}), ("parse_all_ones", {"parse": 0xFFFFFFFF}),
            # content + data wraps; more new blocks than 32 bits count
            ("content_plus_data_wraps", {"data_bytes": M64 - 9095, "scratch_bytes": BIG}),
            ("data_all_ones", {"data_bytes": M64, "scratch_bytes": BIG}),
            ("too_many_blocks", {"data_bytes": 1 << 44, "scratch_bytes": BIG}),
            # the new frame may not lie over the old one, the data or the scratch: its first byte, its last, all of it
            ("new_frame_is_the_frame", {"d_new_frame": 0x10000}),
            ("new_frame_ends_in_the_frame", {"d_new_frame": 0x10000 - 0x8000 + 16}),
            ("new_frame_starts_in_the_frame", {"d_new_frame": 0x10ff0}),
            ("new_frame_around_the_frame", {"d_new_frame": 0xF000, "capacity": 0x4000}),
            ("new_frame_starts_in_the_data", {"d_new_frame": 0x40180}),
            ("new_frame_ends_in_the_data", {"d_new_frame": 0x40000 - 0x8000 + 16}),
            ("new_frame_starts_in_the_scratch", {"d_new_frame": 0x1000100}),
            ("new_frame_ends_in_the_scratch", {"d_new_frame": 0x1000000 - 0x8000 + 16}),
            # nor the data over the scratch
            ("data_starts_in_the_scratch", {"d_data": 0x1000010}), ("data_ends_in_the_scratch", {"d_data": 0x1000000 - 399}),
            ("scratch_one_short", "short")]


@pytest.mark.parametrize("dict_flavour", [False, True])
def test_every_refusal_at_the_call(dict_flavour):
    L = N.lib()
    for what, kw in REFUSALS:
        if kw == "short":
            kw = {"scratch_bytes": int(L.sqz_hip_frame_append_scratch_bytes(3, 9096, 400, 12, 3000 if dict_flavour else 0)) - 1}
        assert call(L, dict_flavour, **kw) == E.EINVAL, what
    # header and index (and record) outside avail
    assert call(L, dict_flavour, avail=32 + 24 + (8 if dict_flavour else 0) - 1) == E.E2BIG
    if dict_flavour:
        for kw in ({"d_dict": None}, {"dict_bytes": 0}, {"dict_bytes": 32768}, {"win_bits": 11, "dict_bytes": 2048}):
            assert call(L, True, **kw) == E.EINVAL, kw


@pytest.mark.parametrize("dict_flavour", [False, True])
def test_enodev_without_a_device(dict_flavour):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    L = N.lib()
    assert call(L, dict_flavour) == E.ENODEV
    # neighbours are not overlaps; what is null may be null when nothing would be read there; an empty frame
    for kw in ({"d_new_frame": 0x11000}, {"d_new_frame": 0x10000 - 0x8000}, {"d_new_frame": 0x1000000 - 0x8000},
               {"d_new_frame": 0x40000 - 0x8000}, {"d_data": 0x1000000 - 400}, {"data_bytes": 0, "d_data": None},
               {"parse": 1}, {"win_bits": 10, "dict_bytes": 1023}, {"n_blocks": 0, "content_bytes": 0},
               {"n_blocks": 0, "content_bytes": 0, "data_bytes": 0, "d_data": None}):
        assert call(L, dict_flavour, **kw) == E.ENODEV, kw


def test_append_frame_refuses_on_the_host_and_names_itself():
    """every error is a ValueError that says append_frame"""
    import torch
    from sqz_amd import frame as F
    info = {"version": 2, "n_blocks": 3, "content_bytes": 2 * 4096 + 904, "block_bytes": 4096, "win_bits": 12}
    d_frame = torch.zeros(64, dtype=torch.uint8)
    for data in (torch.zeros(4, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.uint8), "text", [1, 2, 3], 7, None):
        with pytest.raises(ValueError, match="^append_frame: "):
            F.append_frame(d_frame, data, info=info)
    with pytest.raises(ValueError, match="parse"):
        F.append_frame(d_frame, bytes(4), info=info, parse="eager")
    import sqz_amd
    assert sqz_amd.append_frame is F.append_frame and "append_frame" in sqz_amd.__all__
