"""CPU: the call-level rules of sqz_hip_frame_gather / _gather_dict (include/sqz/sqz.h) -- the scratch function
against a restatement of its formula, every refusal at the call, ENODEV -- on a machine without a device.  The pointers are never followed here."""
import ctypes as C
import errno

import pytest

from sqz_amd import _native as N

E = errno


def up(v):
    return (v + 255) & ~255


def scratch_formula(n, r, max_blocks, bits):
    m, w = min(max_blocks, n), (n + 31) // 32
    decode = up(2 * m * 4) + ((m << bits) + 64) * 4                 # sqz_hip_decode_scratch_bytes(2 m, m << bits)
    return (2 * up(4 * w + 4) + 256 + up(4 * m + 4) + 2 * up(8 * (2 * m + 1)) + 4 * up(8 * m + 4) + up(8 * r + 8)
            + up(4 * r + 4) + up(decode) + up((m << bits) + 16))


def test_scratch_function_is_its_formula_monotone_and_zero_for_bad_block_bits():
    L = N.lib()
    f = L.sqz_hip_frame_gather_scratch_bytes
    for bits in (12, 13, 18, 24):
        for n in (0, 1, 31, 32, 33, 300, 16384):
            for r in (0, 1, 255, 4096, 65536):
                for m in (0, 1, 3, n, n + 5):
                    assert f(n, r, m, bits) == scratch_formula(n, r, m, bits), (n, r, m, bits)
    assert L.sqz_hip_decode_scratch_bytes(6, 3 << 12) == up(24) + ((3 << 12) + 64) * 4
    base = (300, 257, 40, 12)
    for k in range(4):
        for step in (1, 7, 1000):
            more = list(base)
            more[k] += step if k < 3 else min(step, 12)
            assert f(*more) >= f(*base), (k, step)
    for bits in (0, 11, 25, 64):
        assert f(300, 257, 40, bits) == 0


def _args(L, **kw):
    """a call that passes every check at the call (on made-up device pointers, which nothing follows)"""
    n, content, bits, r, m = 3, 9096, 12, 4, 3
    a = {"d_frame": 0x1000, "avail": 1 << 20, "n_blocks": n, "content_bytes": content, "block_bits": bits,
         "d_offset": 0x2000, "d_length": 0x3000, "n_ranges": r, "max_length": 100, "max_blocks": m,
         "d_dict": 0x9000, "dict_bytes": 3000, "d_out": 0x4000, "out_capacity": 400, "d_out_off": 0x5000,
         "d_range_err": 0x6000, "d_blocks_decoded": 0x7000, "d_status": 0x8000, "d_scratch": 0x10000, "scratch_bytes": None}
    a.update(kw)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = int(L.sqz_hip_frame_gather_scratch_bytes(a["n_blocks"], a["n_ranges"], a["max_blocks"], 12))
    return a


def call(L, dict_flavour, **kw):
    a = _args(L, **kw)
    head = (a["d_frame"], a["avail"], a["n_blocks"], a["content_bytes"], a["block_bits"], a["d_offset"], a["d_length"],
            a["n_ranges"], a["max_length"], a["max_blocks"])
    tail = (a["d_out"], a["out_capacity"], a["d_out_off"], a["d_range_err"], a["d_blocks_decoded"], a["d_status"],
            a["d_scratch"], a["scratch_bytes"], None)
    if dict_flavour:
        return L.sqz_hip_frame_gather_dict(*head, a["d_dict"], a["dict_bytes"], *tail)
    return L.sqz_hip_frame_gather(*head, *tail)


REFUSALS = [("block_bits_11", {"block_bits": 11}), ("block_bits_25", {"block_bits": 25}),
            ("n_blocks_is_not_the_contents", {"n_blocks": 4}), ("content_is_not_n_blocks", {"content_bytes": 3 * 4096 + 1}),
            ("null_frame", {"d_frame": None}), ("misaligned_frame", {"d_frame": 0x1008}),
            ("null_scratch", {"d_scratch": None}), ("misaligned_scratch", {"d_scratch": 0x10004}),
            ("null_status", {"d_status": None}), ("null_blocks_decoded", {"d_blocks_decoded": None}),
            ("null_out_off", {"d_out_off": None}), ("null_offset", {"d_offset": None}), ("null_length", {"d_length": None}),
            ("null_range_err", {"d_range_err": None}), ("null_out", {"d_out": None}), ("scratch_one_short", "short")]


@pytest.mark.parametrize("dict_flavour", [False, True])
def test_every_refusal_at_the_call(dict_flavour):
    L = N.lib()
    for what, kw in REFUSALS:
        if kw == "short":
            kw = {"scratch_bytes": int(L.sqz_hip_frame_gather_scratch_bytes(3, 4, 3, 12)) - 1}
        assert call(L, dict_flavour, **kw) == E.EINVAL, what
    # header and index (and record) outside avail
    assert call(L, dict_flavour, avail=32 + 24 + (8 if dict_flavour else 0) - 1) == E.E2BIG
    if dict_flavour:
        for kw in ({"d_dict": None}, {"dict_bytes": 0}, {"dict_bytes": 32768}):
            assert call(L, True, **kw) == E.EINVAL, kw


@pytest.mark.parametrize("dict_flavour", [False, True])
def test_enodev_without_a_device(dict_flavour):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    assert call(N.lib(), dict_flavour) == E.ENODEV
    # what is null may be null when nothing would be read or written there
    for kw in ({"n_ranges": 0, "d_offset": None, "d_length": None, "d_range_err": None}, {"max_blocks": 0, "d_out": None}):
        assert call(N.lib(), dict_flavour, **kw) == E.ENODEV, kw
