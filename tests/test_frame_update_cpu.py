"""CPU: the call-level rules of sqz_hip_frame_update / _update_dict (include/sqz/sqz.h) -- the scratch function against
a restatement of its formula, every refusal at the call, ENODEV -- on a machine without a device.  The pointers are
never followed here.  And what update_frame refuses on the host, before anything is enqueued."""
import errno

import pytest

from sqz_amd import _native as N

E = errno


def up(v):
    return (v + 255) & ~255


def scratch_formula(n, r, max_blocks, bits, D):
    """the header's terms, one by one"""
    m, w = min(max_blocks, n), (n + 31) // 32
    gather = (2 * up(4 * w + 4) + 256 + up(4 * m + 4) + 2 * up(8 * (2 * m + 1)) + 4 * up(8 * m + 4) + up(8 * r + 8)
              + up(4 * r + 4) + up((m << bits) + 16))
    lists = up(8 * r + 8) + 2 * up(8 * (m + 1)) + up(8 * m + 8) + 2 * up(4 * m + 4)
    table = up(8 * (2 * m + 2)) + 2 * up(8 * (2 * m + 1)) + 256
    dict_index = 256 + 2 * up(4 * (D + 64)) if D > 0 else 0
    slabs = up(m * (2 * (1 << bits) + 1024))                         # m * sqz_bound(2^bits)
    decode = up(2 * m * 4) + ((m << bits) + 64) * 4                  # sqz_hip_decode_scratch_bytes(2 m, m << bits)
    encode = up(m * 4) + 2 * ((m << bits) + 64) * 4                  # sqz_hip_encode_scratch_bytes(m, m << bits)
    return gather + lists + table + dict_index + slabs + up(max(decode, encode))


def test_scratch_function_is_its_formula_monotone_and_zero_for_bad_arguments():
    L = N.lib()
    f = L.sqz_hip_frame_update_scratch_bytes
    for bits in (12, 13, 18, 24):
        for n in (0, 1, 31, 32, 33, 300, 16384):
            for r in (0, 1, 255, 4096, 65536):
                for m in (0, 1, 3, n, n + 5):
                    for D in (0, 1, 3000, 32767):
                        assert f(n, r, m, bits, D) == scratch_formula(n, r, m, bits, D), (n, r, m, bits, D)
    assert L.sqz_bound(4096) == 2 * 4096 + 1024
    assert L.sqz_hip_decode_scratch_bytes(6, 3 << 12) == up(24) + ((3 << 12) + 64) * 4
    assert L.sqz_hip_encode_scratch_bytes(3, 3 << 12) == up(12) + 2 * ((3 << 12) + 64) * 4
    base = (300, 257, 40, 12, 100)
    for k in range(5):
        for step in (1, 7, 1000):
            more = list(base)
            more[k] += min(step, 12) if k == 3 else step
            assert f(*more) >= f(*base), (k, step)
    # more than a gather of the same request takes
    assert f(300, 257, 40, 12, 0) > L.sqz_hip_frame_gather_scratch_bytes(300, 257, 40, 12)
    for bits in (0, 11, 25, 64):
        assert f(300, 257, 40, bits, 0) == 0
    assert f(300, 257, 40, 12, 32768) == 0


def _args(L, **kw):
    """a call that passes every check at the call (on made-up device pointers, which nothing follows)"""
    n, content, bits, r, m = 3, 9096, 12, 4, 3
    a = {"d_frame": 0x10000, "avail": 0x1000, "n_blocks": n, "content_bytes": content, "win_bits": 15, "block_bits": bits,
         "d_offset": 0x2000, "d_length": 0x3000, "n_ranges": r, "max_length": 100, "max_blocks": m, "d_data": 0x4000,
         "data_bytes": 400, "d_data_off": 0x5000, "parse": 0, "d_dict": 0x9000, "dict_bytes": 3000,
         "d_new_frame": 0x100000, "capacity": 0x8000, "d_frame_bytes": 0x5800, "d_range_err": 0x6000,
         "d_blocks_encoded": 0x7000, "d_status": 0x8000, "d_scratch": 0x1000000, "scratch_bytes": None, "dict": False}
    a.update(kw)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = int(L.sqz_hip_frame_update_scratch_bytes(a["n_blocks"], a["n_ranges"], a["max_blocks"], 12,
                                                                      a["dict_bytes"] if a["dict"] else 0))
    return a


def call(L, dict_flavour, **kw):
    a = _args(L, dict=dict_flavour, **kw)
    head = (a["d_frame"], a["avail"], a["n_blocks"], a["content_bytes"], a["win_bits"], a["block_bits"], a["d_offset"],
            a["d_length"], a["n_ranges"], a["max_length"], a["max_blocks"], a["d_data"], a["data_bytes"], a["d_data_off"],
            a["parse"])
    tail = (a["d_new_frame"], a["capacity"], a["d_frame_bytes"], a["d_range_err"], a["d_blocks_encoded"], a["d_status"],
            a["d_scratch"], a["scratch_bytes"], None)
    if dict_flavour:
        return L.sqz_hip_frame_update_dict(*head, a["d_dict"], a["dict_bytes"], *tail)
    return L.sqz_hip_frame_update(*head, *tail)


REFUSALS = [("block_bits_11", {"block_bits": 11}), ("block_bits_25", {"block_bits": 25}),
            ("win_bits_9", {"win_bits": 9}), ("win_bits_16", {"win_bits": 16}),
            ("n_blocks_is_not_the_contents", {"n_blocks": 4}), ("content_is_not_n_blocks", {"content_bytes": 3 * 4096 + 1}),
            ("null_frame", {"d_frame": None}), ("misaligned_frame", {"d_frame": 0x10008}),
            ("null_scratch", {"d_scratch": None}), ("misaligned_scratch", {"d_scratch": 0x1000004}),
            ("null_status", {"d_status": None}), ("null_blocks_encoded", {"d_blocks_encoded": None}),
            ("null_data_off", {"d_data_off": None}), ("null_offset", {"d_offset": None}), ("null_length", {"d_length": None}),
            ("null_range_err", {"d_range_err": None}), ("null_data", {"d_data": None}),
            ("null_new_frame", {"d_new_frame": None}), ("misaligned_new_frame", {"d_new_frame": 0x100008}),
            ("null_frame_bytes", {"d_frame_bytes": None}), ("parse_2", {"parse": 2}), ("parse_all_ones", {"parse": 0xFFFFFFFF}),
            # the new frame may not lie over the old one or over the scratch: its first byte, its last, all of it
            ("new_frame_is_the_frame", {"d_new_frame": 0x10000}),
            ("new_frame_ends_in_the_frame", {"d_new_frame": 0x10000 - 0x8000 + 16}),
            ("new_frame_starts_in_the_frame", {"d_new_frame": 0x10ff0}),
            ("new_frame_around_the_frame", {"d_new_frame": 0xF000, "capacity": 0x4000}),
            ("new_frame_starts_in_the_scratch", {"d_new_frame": 0x1000100}),
            ("new_frame_ends_in_the_scratch", {"d_new_frame": 0x1000000 - 0x8000 + 16}),
            ("scratch_one_short", "short")]


@pytest.mark.parametrize("dict_flavour", [False, True])
def test_every_refusal_at_the_call(dict_flavour):
    L = N.lib()
    for what, kw in REFUSALS:
        if kw == "short":
            kw = {"scratch_bytes": int(L.sqz_hip_frame_update_scratch_bytes(3, 4, 3, 12, 3000 if dict_flavour else 0)) - 1}
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
    # neighbours are not overlaps; what is null may be null when nothing would be read or written there
    for kw in ({"d_new_frame": 0x11000}, {"d_new_frame": 0x10000 - 0x8000}, {"d_new_frame": 0x1000000 - 0x8000},
               {"n_ranges": 0, "d_offset": None, "d_length": None, "d_range_err": None},
               {"data_bytes": 0, "d_data": None}, {"parse": 1}, {"win_bits": 10, "dict_bytes": 1023}):
        assert call(L, dict_flavour, **kw) == E.ENODEV, kw


def test_update_frame_refuses_on_the_host_and_names_itself():
    """sequences are checked here as gather_frame checks them; every error is a ValueError that says update_frame"""
    import torch
    from sqz_amd import frame as F
    content = 2 * 4096 + 904
    info = {"version": 2, "n_blocks": 3, "content_bytes": content, "block_bytes": 4096, "win_bits": 12}
    d_frame = torch.zeros(64, dtype=torch.uint8)
    dev = torch.zeros(2, dtype=torch.int64)
    data = bytes(40)
    cases = [
        (([content - 3], [4], data), {}),                                   # leaves the content
        (([content + 1], [0], data), {}),                                   # starts behind it
        (([0], [10], data), {"max_length": 9}),                             # longer than max_length
        (([0, 8], [4], data), {}),                                          # as many lengths as offsets
        (([-1], [4], data), {}), (([0], [1 << 64], data), {}),              # not 0 .. 2^64 - 1
        ((dev, dev, data), {}),                                             # device tensors: max_length is required
        ((dev.to(torch.int32), [4, 4], data), {}),                          # offsets of another type, or shape
        ((dev.reshape(1, 2), [4, 4], data), {}),
        (([0], [4], torch.zeros(4, dtype=torch.int32)), {}),                # data that is not uint8, or not flat
        (([0], [4], torch.zeros(2, 2, dtype=torch.uint8)), {}),
    ]
    for args, kw in cases:
        with pytest.raises(ValueError, match="^update_frame: "):
            F.update_frame(d_frame, *args, info=info, **kw)
    with pytest.raises(ValueError, match="parse"):
        F.update_frame(d_frame, [0], [4], data, info=info, parse="eager")
