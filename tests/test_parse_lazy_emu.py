"""CPU: the lazy instantiation of index_parse_kernel (sqz_amd/csrc/lz77_index.hip) on the wave emulator.

  * the kernel alone on synthetic match tables (dense literals, 30 % matches, some of 200-257), against a
    serial walk of the rule written here.  The tables carry, on the path, what the lazy walk can get wrong: a
    position that gives way at a tile's last position (its successor is the next tile's first word), at every
    chunk's last position (the successor is the next lane's first word), three in a row across a chunk edge, a
    match at n-3 in front of position n-2 (a literal whatever the table says there: no giving way), equal
    lengths (no giving way); block lengths around one and two tiles, and blocks of 0, 1 and 2 bytes.
  * match + lazy parse on real text against tests/lazy_model.py.
  * the greedy launcher on the same tables still gives the greedy walk."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lazy_model as LM
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
TOK_MATCH = 0x80000000


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(EMU, "libsqz_emu_parse_lazy.so")
    deps = [os.path.join(EMU, f) for f in ("emu_runtime.cpp", "emu_parse_lazy.cpp", "hip/hip_runtime.h")] + \
           [os.path.join(CSRC, f) for f in ("sqz_device.h", "sqz_kernels.h", "lz77_index.hip")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-I" + EMU,
                               "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                               "-Wno-attributes", os.path.join(EMU, "emu_runtime.cpp"),
                               os.path.join(EMU, "emu_parse_lazy.cpp"), "-o", out])
    L = C.CDLL(out)
    L.emu_index_match.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                  C.c_uint32, C.c_uint64]
    L.emu_index_parse.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_uint64, C.c_int]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _layout(blocks):
    sizes = [len(b) for b in blocks]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    data = np.frombuffer(b"".join(blocks) + b"\0", np.uint8).copy()      # (+1: never an empty array)
    return data, offs, int(offs[-1])


def _parse(lib, data, offs, total, match, lazy):
    n = len(offs) - 1
    toks = np.full(total + 1, 0xCCCCCCCC, np.uint32)
    counts = np.full(n, 0xCCCCCCCC, np.uint32)
    assert lib.emu_index_parse(_p(data), _p(offs), n, _p(match), _p(toks), _p(counts), total, int(lazy)) == 0
    return toks, counts


def _synthetic(n, seed):
    """bytes and a match table for n positions: literals (the byte itself), 30 % matches of which 5 % are
    200..257 long, never reaching past the end; the last two words are never to be read"""
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


def _len(src, m, i):
    return int(m[i]) >> 16 if i + 2 < len(src) else 0


def _walk(src, m, lazy):
    """the rule, one token after the other -> (token words, positions that gave way)"""
    n = len(src)
    out, gave = [], []
    i = 0
    while i < n:
        li = _len(src, m, i)
        if lazy and li >= 3 and i + 1 < n and _len(src, m, i + 1) > li:
            out.append(int(src[i]))
            gave.append(i)
            i += 1
        elif li != 0:
            out.append(TOK_MATCH | int(m[i]))
            i += li
        else:
            out.append(int(src[i]) if i + 2 >= n else int(m[i]) & 0xFF)
            i += 1
    return np.array(out, np.uint32), gave


def _literals(src, m, lo, hi):
    lo = max(lo, 0)
    m[lo:hi] = src[lo:hi]


def _match(length, dist=7):
    return (length << 16) | dist


def _check(lib, tables):
    """both launchers on the same tables against the two walks; nothing written behind a block's tokens"""
    data, offs, total = _layout([s.tobytes() for s, _ in tables])
    match = np.concatenate([m for _, m in tables] + [np.zeros(1, np.uint32)])
    for lazy in (True, False):
        toks, counts = _parse(lib, data, offs, total, match, lazy)
        for k, (src, m) in enumerate(tables):
            want, _ = _walk(src, m, lazy)
            assert int(counts[k]) == len(want), (lazy, k, len(src), int(counts[k]), len(want))
            got = toks[int(offs[k]):int(offs[k]) + len(want)]
            assert (got == want).all(), (lazy, k, len(src), int(np.argmax(got != want)))
            assert (toks[int(offs[k]) + len(want):int(offs[k + 1])] == 0xCCCCCCCC).all(), (lazy, k, len(src))


def _edge_table(n, seed, T):
    """a synthetic table of n >= T - 1 positions with the cases planted on the path; -> (src, m, what to find)"""
    src, m = _synthetic(n, seed)
    expect = {"gave": [], "kept": []}
    # a run of literals longer than the longest match puts the path on every position behind it
    _literals(src, m, 100, 420)
    m[382:386] = [_match(3), _match(4), _match(5), _match(6)]            # three in a row across the chunk edge 383 | 384
    expect["gave"] += [382, 383, 384]
    _literals(src, m, 391, 700)
    m[660], m[661] = _match(5), _match(5, 9)                             # equal lengths: the first one stays
    expect["kept"].append(660)
    for p in range(T - 1, n, T):                                         # a tile's last position
        if p + 1 + 9 <= n and p + 1 < n - 2:
            _literals(src, m, p - 300, p)
            m[p], m[p + 1] = _match(5), _match(9)
            expect["gave"].append(p)
    # a match at n-3: position n-2 is a literal whatever its table word says (0xDEADBEEF: a huge length)
    if n >= T - 1:
        _literals(src, m, n - 300, n - 3)
        m[n - 3] = _match(3)
        expect["kept"].append(n - 3)
    return src, m, expect


def test_lazy_parse_at_the_tile_edges(lib):
    T = lib.emu_parse_tile()
    assert T == 2048 and lib.emu_parse_chunk() == 32
    # (behind position 2T - 1 the lengths around 2T leave no room for a longer match: 3T + 1 has it)
    lengths = [k * T + d for k in (1, 2) for d in (-1, 0, 1, 2, 3)] + [3 * T + 1]
    built = [_edge_table(n, 500 + k, T) for k, n in enumerate(lengths)]
    seen_tile_last = set()
    for n, (src, m, expect) in zip(lengths, built):
        toks, gave = _walk(src, m, True)
        assert set(expect["gave"]) <= set(gave), (n, expect["gave"])
        assert not set(expect["kept"]) & set(gave), (n, expect["kept"])
        assert LM.longest_chain(gave) >= 3
        seen_tile_last |= {p for p in gave if p % T == T - 1}
        # n-3 is on the path and its match is taken: the block's last token
        assert int(toks[-1]) == TOK_MATCH | _match(3), n
    assert seen_tile_last == {T - 1, 2 * T - 1}
    _check(lib, [(s, m) for s, m, _ in built])


def test_lazy_parse_gives_way_at_every_chunks_last_position(lib):
    T = lib.emu_parse_tile()
    n = 3 * T + 5
    src, m = _synthetic(n, 600)
    _literals(src, m, 0, n)
    last = np.arange(31, n - 12, 32)
    m[last] = _match(4)
    m[last + 1] = _match(6, 11)
    toks, gave = _walk(src, m, True)
    assert gave == list(last) and T - 1 in gave and 2 * T - 1 in gave
    _check(lib, [(src, m)])


def test_lazy_parse_on_plain_synthetic_tables_and_short_blocks(lib):
    T = lib.emu_parse_tile()
    lengths = [3 * T + 777, 0, 1, 2, 3, 4, 5, 63, 64, 65]
    tables = [_synthetic(n, 700 + k) for k, n in enumerate(lengths)]
    assert len(_walk(*tables[0], True)[1]) > 20                         # the random table gives way now and then
    _check(lib, tables)


def _sorted_positions(block):
    a = np.frombuffer(block, np.uint8).astype(np.uint32)
    if len(a) < 3:
        return np.zeros(0, np.uint32)
    key = (a[:-2] << 16) | (a[1:-1] << 8) | a[2:]
    return np.argsort(key, kind="stable").astype(np.uint32)


def test_match_and_lazy_parse_give_the_models_tokens(lib):
    window = 1 << 10
    block = O.corpus("laozi.txt")[:9000]
    data, offs, total = _layout([block])
    srt = np.zeros(total + 1, np.uint32)
    s = _sorted_positions(block)
    srt[:len(s)] = s
    match = np.full(total + 1, 0xDEADBEEF, np.uint32)
    assert lib.emu_index_match(_p(data), _p(offs), 1, window, _p(srt), _p(match), 1, total) == 0
    tab = LM.table(block, window)
    greedy, _ = LM.parse(block, window, False, tab)
    assert (greedy == O.tokens(block, window)).all()                     # the model's greedy branch is the oracle's
    lazy, gave = LM.parse(block, window, True, tab)
    assert len(gave) > 20 and len(lazy) != len(greedy)
    e, back, _ = O.decode(LM.stream(lazy), header=False, nbytes=len(block))
    assert e == 0 and back == block
    for is_lazy, want in ((True, lazy), (False, greedy)):
        toks, counts = _parse(lib, data, offs, total, match, is_lazy)
        assert int(counts[0]) == len(want), (is_lazy, int(counts[0]), len(want))
        assert (toks[:len(want)] == want).all(), (is_lazy, int(np.argmax(toks[:len(want)] != want)))
        assert (toks[len(want):total] == 0xCCCCCCCC).all()
