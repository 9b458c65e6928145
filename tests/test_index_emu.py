"""CPU: index_match_kernel and index_parse_kernel themselves (sqz_amd/csrc/lz77_index.hip), compiled by g++
against tests/emu/hip/hip_runtime.h and run lane by lane on the CPU wave emulator.

  * match + parse against the oracle's tokens, windows 2^15 and 2^10.  The emulator runs workgroups of up to
    8 waves and index_sort_kernel has 16, so the sorted positions come from numpy: a stable argsort of the
    24-bit big-endian key of every position that has one -- what the sort kernel promises.
  * index_parse_kernel alone on synthetic match tables (dense literals, 30 % matches, 5 % of those 200-257
    long, so that tokens reach across chunks and tiles), against a serial greedy walk written here; and on
    block lengths around one and two parse tiles, where the last two positions (literals taken from the
    bytes, not from the table) fall on either side of a tile's edge.

This pins the kernels' LOGIC without a GPU; gfx950 code generation, LDS ordering and timing are the -m gpu
tests' (test_index_parse_shapes.py, test_index_sort_shapes.py, test_gpu_parity.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
TOK_MATCH = 0x80000000


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(EMU, "libsqz_emu_index.so")
    deps = [os.path.join(EMU, f) for f in ("emu_runtime.cpp", "emu_index.cpp", "hip/hip_runtime.h")] + \
           [os.path.join(CSRC, f) for f in ("sqz_device.h", "sqz_kernels.h", "lz77_index.hip")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-I" + EMU,
                               "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                               "-Wno-attributes", os.path.join(EMU, "emu_runtime.cpp"),
                               os.path.join(EMU, "emu_index.cpp"), "-o", out])
    L = C.CDLL(out)
    L.emu_index_match.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                  C.c_uint32, C.c_uint64]
    L.emu_index_parse.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _layout(blocks):
    sizes = [len(b) for b in blocks]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    data = np.frombuffer(b"".join(blocks) + b"\0", np.uint8).copy()      # (+1: never an empty array)
    return data, offs, int(offs[-1])


def _sorted_positions(block):
    """what index_sort_kernel leaves: positions 0..n-3 by their 3-byte prefix, byte 0 most significant,
    positions ascending among equal prefixes"""
    a = np.frombuffer(block, np.uint8).astype(np.uint32)
    if len(a) < 3:
        return np.zeros(0, np.uint32)
    key = (a[:-2] << 16) | (a[1:-1] << 8) | a[2:]
    return np.argsort(key, kind="stable").astype(np.uint32)


def _parse(lib, data, offs, total, match):
    n = len(offs) - 1
    toks = np.full(total + 1, 0xCCCCCCCC, np.uint32)
    counts = np.full(n, 0xCCCCCCCC, np.uint32)
    assert lib.emu_index_parse(_p(data), _p(offs), n, _p(match), _p(toks), _p(counts), total) == 0
    return toks, counts


def _tokens(lib, blocks, window):
    data, offs, total = _layout(blocks)
    srt = np.zeros(total + 1, np.uint32)
    for k, b in enumerate(blocks):
        s = _sorted_positions(b)
        srt[int(offs[k]):int(offs[k]) + len(s)] = s
    match = np.full(total + 1, 0xDEADBEEF, np.uint32)
    assert lib.emu_index_match(_p(data), _p(offs), len(blocks), window, _p(srt), _p(match), 1, total) == 0
    toks, counts = _parse(lib, data, offs, total, match)
    return [toks[int(offs[k]):int(offs[k]) + int(counts[k])] for k in range(len(blocks))], toks, offs, counts


def _inputs():
    return [O.zipf_block(0, 20000), O.zipf_block(1, 70001), b"abcabc" * 50, bytes(5000),
            O.corpus("laozi.txt")[:9000], b"ab", b""]


@pytest.mark.parametrize("window", [1 << 15, 1 << 10])
def test_match_and_parse_give_the_oracles_tokens(lib, window):
    blocks = _inputs()
    got, toks, offs, counts = _tokens(lib, blocks, window)
    for k, b in enumerate(blocks):
        want = O.tokens(b, window)
        assert int(counts[k]) == len(want), (k, len(b), int(counts[k]), len(want))
        assert (got[k] == want).all(), (k, len(b), int(np.argmax(got[k] != want)))
        # nothing is written behind a block's last token
        assert (toks[int(offs[k]) + len(want):int(offs[k + 1])] == 0xCCCCCCCC).all(), (k, len(b))


def _synthetic(n, seed):
    """bytes and a match table for a block of n positions: literals (the byte itself), 30 % matches of which
    5 % are 200..257 long, never reaching past the block's end; the last two words are never to be read"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, n, dtype=np.uint8)
    m = src.astype(np.uint32)
    is_match = rng.random(n) < 0.30
    long_one = rng.random(n) < 0.05
    length = np.where(long_one, rng.integers(200, 258, n), rng.integers(3, 20, n)).astype(np.int64)
    length = np.minimum(length, n - np.arange(n))
    dist = rng.integers(1, 32768, n).astype(np.uint32)
    use = is_match & (length >= 3)
    m[use] = (length[use].astype(np.uint32) << 16) | dist[use]
    if n >= 1:
        m[max(n - 2, 0):] = 0xDEADBEEF
    return src, m


def _greedy(src, m):
    n = len(src)
    out = []
    i = 0
    while i < n:
        w = int(m[i]) if i + 2 < n else int(src[i])
        if w >> 16:
            out.append(TOK_MATCH | w)
            i += w >> 16
        else:
            out.append(w & 0xFF)
            i += 1
    return np.array(out, np.uint32)


def _check_parse(lib, lengths, seed):
    tables = [_synthetic(n, seed + k) for k, n in enumerate(lengths)]
    data, offs, total = _layout([s.tobytes() for s, _ in tables])
    match = np.concatenate([m for _, m in tables] + [np.zeros(1, np.uint32)])
    toks, counts = _parse(lib, data, offs, total, match)
    for k, (src, m) in enumerate(tables):
        want = _greedy(src, m)
        assert int(counts[k]) == len(want), (k, lengths[k], int(counts[k]), len(want))
        got = toks[int(offs[k]):int(offs[k]) + len(want)]
        assert (got == want).all(), (k, lengths[k], int(np.argmax(got != want)))
        assert (toks[int(offs[k]) + len(want):int(offs[k + 1])] == 0xCCCCCCCC).all(), (k, lengths[k])


def test_parse_alone_three_tiles_and_a_ragged_rest(lib):
    T = lib.emu_parse_tile()
    _check_parse(lib, [3 * T + 777, 3 * T + 5], seed=100)


def test_parse_alone_at_the_tile_edges(lib):
    T = lib.emu_parse_tile()
    # k * T - 1, k * T, k * T + 1 positions, and the two lengths that put position bytes-2 / bytes-1 in front
    # of the edge with the block's end behind it
    _check_parse(lib, [k * T + d for k in (1, 2) for d in (-1, 0, 1, 2, 3)], seed=200)


def test_parse_alone_short_blocks(lib):
    _check_parse(lib, [0, 1, 2, 3, 4, 63, 64, 65], seed=300)


def test_a_zero_length_field_advances_by_one(lib):
    """a word with no length but a distance is not something index_match_kernel writes; the parse must still
    step over it (as a literal of its low byte) instead of standing still"""
    T = lib.emu_parse_tile()
    n = T + 100
    src, m = _synthetic(n, 400)
    m[np.arange(5, n - 2, 7)] = 0x00004321
    data, offs, total = _layout([src.tobytes()])
    toks, counts = _parse(lib, data, offs, total, np.concatenate([m, np.zeros(1, np.uint32)]))
    want = _greedy(src, m)
    assert int(counts[0]) == len(want)
    assert (toks[:len(want)] == want).all()
