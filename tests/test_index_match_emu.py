"""CPU: index_match_kernel itself (sqz_amd/csrc/lz77_index.hip) on the wave emulator, at the shapes its page pipeline can
get wrong (tests/match_shapes.py): blocks shorter than 16 bytes and around the shifted tail load, counts of one page, one
rank over and two pages, a workgroup's edge, one ragged launch whose long block keeps the register double buffer running
for dozens of pages per wave, and the data that takes each path of the kernel (shared walk, several runs, own walks).

match[] is compared WORD FOR WORD with a model written here: for every position that has a 3-byte prefix, the earlier
positions with the same prefix inside the window, nearest first, the first strictly longer match kept, lengths capped at
257 and at the block's end; len << 16 | dist, or the position's byte where nothing of 3 bytes or more matches.  The words
of the last two positions, and everything outside the blocks, must stay untouched.  Then index_parse_kernel runs over
that table and the tokens are held against the oracle's.  Windows 2^10 and 2^15."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import match_shapes as shapes
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
LEN_MAX = 257
UNTOUCHED = 0xDEADBEEF

CASES = shapes.cases()


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


def _sorted_positions(block):
    """what index_sort_kernel leaves: positions 0..n-3 by their 3-byte prefix, byte 0 most significant,
    positions ascending among equal prefixes"""
    a = np.frombuffer(block, np.uint8).astype(np.uint32)
    if len(a) < 3:
        return np.zeros(0, np.uint32)
    key = (a[:-2] << 16) | (a[1:-1] << 8) | a[2:]
    return np.argsort(key, kind="stable").astype(np.uint32)


def _model(block, window):
    """match words of positions 0..n-3"""
    a = np.frombuffer(block, np.uint8)
    n = len(a)
    out = np.zeros(max(n - 2, 0), np.uint32)
    runs = {}
    for i in range(n - 2):
        cap = min(n - i, LEN_MAX)
        reach = min(i, window - 1)
        best, dist = 0, 0
        earlier = runs.setdefault(block[i:i + 3], [])
        mine = a[i:i + cap]
        for p in reversed(earlier):                      # nearest first
            if i - p > reach or best >= cap:
                break
            if best >= 3 and a[p + best] != a[i + best]:
                continue                                 # cannot be strictly longer
            diff = np.flatnonzero(a[p:p + cap] != mine)
            k = int(diff[0]) if len(diff) else cap
            if k > best:
                best, dist = k, i - p
        earlier.append(i)
        out[i] = (best << 16) | dist if best >= 3 else int(a[i])
    return out


_MODEL = {}


def _model_of(name, k, block, window):
    """the model's words, worked out once per (case, block, window)"""
    key = (name, k, window)
    if key not in _MODEL:
        w = _model(block, window)
        w.setflags(write=False)
        _MODEL[key] = w
    return _MODEL[key]


def _groups(blocks):
    """match_groups as the encoder sets it: one workgroup per KB of the AVERAGE block (match_groups_for, abi.hip)"""
    avg = sum(len(b) for b in blocks) // len(blocks)
    return min(max((avg + 1023) // 1024, 1), 65535)


@pytest.mark.parametrize("window", [1 << 10, 1 << 15])
@pytest.mark.parametrize("name", list(CASES))
def test_match_words_are_the_models_and_the_tokens_the_oracles(lib, name, window):
    blocks = CASES[name]
    sizes = [len(b) for b in blocks]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    total = int(offs[-1])
    data = np.frombuffer(b"".join(blocks) + b"\0", np.uint8).copy()
    srt = np.zeros(total + 1, np.uint32)
    for k, b in enumerate(blocks):
        s = _sorted_positions(b)
        srt[int(offs[k]):int(offs[k]) + len(s)] = s
    for groups in sorted({1, _groups(blocks)}):
        match = np.full(total + 1, UNTOUCHED, np.uint32)
        assert lib.emu_index_match(_p(data), _p(offs), len(blocks), window, _p(srt), _p(match), groups, total) == 0
        for k, b in enumerate(blocks):
            lo, n = int(offs[k]), len(b)
            want = _model_of(name, k, b, window)
            got = match[lo:lo + len(want)]
            assert (got == want).all(), (name, groups, k, n, int(np.argmax(got != want)))
            assert (match[lo + len(want):lo + n] == UNTOUCHED).all(), (name, groups, k, n)
        assert match[total] == UNTOUCHED
        toks = np.full(total + 1, 0xCCCCCCCC, np.uint32)
        counts = np.full(len(blocks), 0xCCCCCCCC, np.uint32)
        assert lib.emu_index_parse(_p(data), _p(offs), len(blocks), _p(match), _p(toks), _p(counts), total) == 0
        for k, b in enumerate(blocks):
            want = O.tokens(b, window)
            assert int(counts[k]) == len(want), (name, groups, k, len(b), int(counts[k]), len(want))
            got = toks[int(offs[k]):int(offs[k]) + len(want)]
            assert (got == want).all(), (name, groups, k, len(b), int(np.argmax(got != want)))
