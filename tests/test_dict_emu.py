"""CPU: the shared-dictionary kernels on the wave emulator, against tests/dict_model.py.

  * dict_match_kernel behind index_match_kernel (sqz_amd/csrc/lz77_index.hip): the merged match table equals
    oracle_lib.match_at(Dct + B, D + i, window) at EVERY position, and both parse kernels over it give the model's
    tokens.  The inputs are dict_model.cases(): the corners (a source in the dictionary's last two bytes, one that
    straddles its end, a periodic copy out of it, a match of 257, a tie the block keeps, window 2^10 with D = 1023,
    D = 32767, D of 1, 2 and 3, blocks of 0..3 bytes) are asserted to be on the path first.
  * the decoder (sqz_amd/csrc/decode.hip): the entropy kernels with a history, 1, 2, 4 and 8 waves, and the
    dictionary instantiation of lz_expand_kernel, against the model's expander; a distance that reaches one byte in
    front of the dictionary is EINVAL, the farthest one inside it is not.

What the emulator does NOT see, and tests/test_dict_gpu.py does: the emulator runs workgroups of up to 8 waves, so
dict_match_kernel is built here with SQZ_DICT_THREADS = 512 (the shipped kernel's 1,024-thread stride through the
LDS load loops and the positions runs on the GPU only); and the sorted positions of the dictionary come from numpy
here, so index_sort_kernel's result for the dictionary as a one-block batch (positions in the low 16 bits of its
first buffer, ascending inside a run, nothing for D < 3) is checked on the GPU only."""
import ctypes as C
import errno
import os
import subprocess

import numpy as np
import pytest

import dict_model as DM
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sqz_amd", "csrc")
TOK_MATCH = DM.TOK_MATCH


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(EMU, "libsqz_emu_dict.so")
    deps = [os.path.join(EMU, f) for f in ("emu_runtime.cpp", "emu_dict.cpp", "hip/hip_runtime.h")] + \
           [os.path.join(CSRC, f) for f in ("sqz_device.h", "sqz_tree.h", "sqz_kernels.h", "lz77_index.hip", "decode.hip")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-I" + EMU,
                               "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                               "-Wno-attributes", os.path.join(EMU, "emu_runtime.cpp"),
                               os.path.join(EMU, "emu_dict.cpp"), "-o", out])
    L = C.CDLL(out)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.emu_index_match.argtypes = [vp, vp, u32, u32, vp, vp, u32, u64]
    L.emu_dict_match.argtypes = [vp, vp, u32, u32, vp, u32, vp, vp, u64]
    L.emu_index_parse.argtypes = [vp, vp, u32, vp, vp, vp, u64, C.c_int]
    L.emu_expand_dict.argtypes = [vp, vp, vp, vp, u32, vp, u32]
    L.emu_decode_dict.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp, C.c_int, vp, u32]
    return L


@pytest.fixture(scope="module")
def cases():
    """dict_model.cases() with the model's tables and tokens, computed once"""
    out = []
    for name, window, dct, blocks, want in DM.cases(O.corpus("laozi.txt"), O.corpus("confucius.txt")):
        tabs = [DM.table(dct, b, window) for b in blocks]
        toks = {lazy: [DM.tokens(dct, b, window, lazy, t) for b, t in zip(blocks, tabs)] for lazy in (False, True)}
        assert want <= DM.corners(toks[False][0], len(dct)), (name, want - DM.corners(toks[False][0], len(dct)))
        out.append((name, window, dct, blocks, tabs, toks))
    return out


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _layout(blocks):
    offs = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.uint64)
    data = np.frombuffer(b"".join(blocks) + b"\0", np.uint8).copy()
    return data, offs, int(offs[-1])


def _sorted_positions(block):
    a = np.frombuffer(block, np.uint8).astype(np.uint32)
    if len(a) < 3:
        return np.zeros(0, np.uint32)
    key = (a[:-2] << 16) | (a[1:-1] << 8) | a[2:]
    return np.argsort(key, kind="stable").astype(np.uint32)


def _merged_table(lib, window, dct, blocks):
    data, offs, total = _layout(blocks)
    srt = np.zeros(total + 64, np.uint32)
    for k, b in enumerate(blocks):
        s = _sorted_positions(b)
        srt[int(offs[k]):int(offs[k]) + len(s)] = s
    match = np.full(total + 64, 0xDEADBEEF, np.uint32)
    assert lib.emu_index_match(_p(data), _p(offs), len(blocks), window, _p(srt), _p(match), 1, total) == 0
    plain = match.copy()
    dsrt = np.full(len(dct) + 64, 0xCCCCCCCC, np.uint32)             # (what lies behind the D - 2 entries is never used)
    s = _sorted_positions(dct)
    dsrt[:len(s)] = s
    d = np.frombuffer(dct, np.uint8).copy()
    assert lib.emu_dict_match(_p(data), _p(offs), len(blocks), window, _p(d), len(dct), _p(dsrt), _p(match), total) == 0
    return data, offs, total, plain, match


def test_the_corners_are_on_the_path(cases):
    seen = set()
    for name, window, dct, blocks, tabs, toks in cases:
        seen |= DM.corners(toks[False][0], len(dct))
        if name == "long_and_tie":
            assert len(DM.ties_kept_in_block(dct, blocks[0], window, toks[False][0])) > 0
        if name == "w10":                                  # a later position has lost the front of the dictionary
            far = [(o, ds) for o, ln, ds, s in DM.sources(toks[False][0], len(dct)) if s < 0 and o > 0]
            assert far and all(ds <= window - 1 for _, ds in far)
            # position 1 is the dictionary's position 0, at distance 1024: a window twice as large would take it
            assert O.match_at(dct + blocks[0], len(dct) + 1, 2 * window) == (257, 1024)
            assert tabs[0][0][1] < 257 and tabs[0][1][1] != 1024
    assert {"source_at_D-1", "source_at_D-2", "straddle", "periodic_from_dict", "first_token", "len_257"} <= seen


def test_dict_match_gives_the_models_table_at_every_position(lib, cases):
    assert lib.emu_dict_threads() == 512
    for name, window, dct, blocks, tabs, toks in cases:
        data, offs, total, plain, match = _merged_table(lib, window, dct, blocks)
        changed = 0
        for k, (b, (L, D)) in enumerate(zip(blocks, tabs)):
            lo = int(offs[k])
            want = np.where(L >= 3, (L.astype(np.uint32) << 16) | D.astype(np.uint32), np.frombuffer(b, np.uint8))
            n = max(len(b) - 2, 0)
            got = match[lo:lo + n]
            assert (got == want[:n]).all(), (name, k, int(np.argmax(got != want[:n])))
            # the last two positions have no word, and nothing behind the block is touched
            assert (match[lo + n:lo + len(b)] == plain[lo + n:lo + len(b)]).all(), (name, k)
            changed += int((got != plain[lo:lo + n]).sum())
        assert (match[total:] == 0xDEADBEEF).all()
        assert changed > 0, name                            # the dictionary did win somewhere


def test_both_parses_over_the_merged_table_give_the_models_tokens(lib, cases):
    for name, window, dct, blocks, tabs, toks in cases:
        data, offs, total, plain, match = _merged_table(lib, window, dct, blocks)
        for lazy in (False, True):
            out = np.full(total + 1, 0xCCCCCCCC, np.uint32)
            counts = np.full(len(blocks), 0xCCCCCCCC, np.uint32)
            assert lib.emu_index_parse(_p(data), _p(offs), len(blocks), _p(match), _p(out), _p(counts), total, int(lazy)) == 0
            for k, want in enumerate(toks[lazy]):
                assert int(counts[k]) == len(want), (name, lazy, k)
                assert (out[int(offs[k]):int(offs[k]) + len(want)] == want).all(), (name, lazy, k)


def _expand(lib, dct, blocks, toks):
    data, offs, total = _layout(blocks)
    words = np.zeros(total + 1, np.uint32)
    counts = np.zeros(len(blocks), np.uint32)
    for k, t in enumerate(toks):
        words[int(offs[k]):int(offs[k]) + len(t)] = t
        counts[k] = len(t)
    out = np.full(total + 8, 0xEE, np.uint8)
    d = np.frombuffer(dct, np.uint8).copy()
    assert lib.emu_expand_dict(_p(words), _p(counts), _p(out), _p(offs), len(blocks), _p(d), len(dct)) == 0
    assert (out[total:] == 0xEE).all()
    return out[:total].tobytes()


def test_expand_with_a_dictionary_gives_the_models_bytes(lib, cases):
    for name, window, dct, blocks, tabs, toks in cases:
        for lazy in (False, True):
            want = b"".join(DM.expand(t, dct) for t in toks[lazy])
            assert want == b"".join(blocks)
            assert _expand(lib, dct, blocks, toks[lazy]) == want, (name, lazy)
    # hand-made tokens: a long periodic copy whose first period is dictionary bytes; an own-lane copy (short, source
    # in the dictionary) next to a whole-wave one; a copy that ends exactly at the dictionary's end
    dct = b"0123456789abcdefXYZ"
    toks = np.array([TOK_MATCH | (200 << 16) | 3,           # XYZXYZ... from D-3: periodic, starts in the dictionary
                     ord("-"),
                     TOK_MATCH | (5 << 16) | (201 + 19),    # "01234": the farthest source, distance = position + D
                     TOK_MATCH | (19 << 16) | (206 + 19),   # the whole dictionary, ending at its end
                     TOK_MATCH | (40 << 16) | (225 + 2),    # "YZ" then the block's own bytes: a straddle
                     ord("."), TOK_MATCH | (3 << 16) | 1], np.uint32)
    want = DM.expand(toks, dct)
    assert want.startswith(b"XYZXYZ") and want[201:206] == b"01234" and want[206:225] == dct and want[225:229] == b"YZXY"
    assert _expand(lib, dct, [want], [toks]) == want


def _decode(lib, dct, streams, sizes, waves):
    n = len(streams)
    in_off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.uint64)
    comp = np.frombuffer(b"".join(streams) + bytes(8), np.uint8).copy()
    out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    total = int(out_off[-1])
    out = np.full(total + 8, 0xEE, np.uint8)
    words = np.zeros(total + 64, np.uint32)
    counts = np.zeros(n, np.uint32)
    err = np.full(n, -1, np.int32)
    d = np.frombuffer(dct, np.uint8).copy()
    assert lib.emu_decode_dict(_p(comp), _p(in_off), n, _p(out), _p(out_off), _p(words), _p(counts), _p(err), waves,
                               _p(d), len(dct)) == 0
    assert (out[total:] == 0xEE).all()
    return out[:total].tobytes(), err


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_decode_with_a_history(lib, cases, waves):
    for name, window, dct, blocks, tabs, toks in cases:
        if name == "w15_full" and waves != 1:               # (the emulator's time: the large case once)
            continue
        for lazy in (False, True):
            streams = [DM.LM.stream(t) for t in toks[lazy]]
            got, err = _decode(lib, dct, streams, [len(b) for b in blocks], waves)
            assert (err == 0).all() and got == b"".join(blocks), (name, lazy, err.tolist())


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_decoder_refuses_a_distance_in_front_of_the_dictionary(lib, waves):
    dct = b"0123456789"
    ok = np.array([ord("a"), ord("b"), TOK_MATCH | (4 << 16) | 12, ord("c")], np.uint32)      # position 2 + D: "0123"
    bad = np.array([ord("a"), ord("b"), TOK_MATCH | (4 << 16) | 13, ord("c")], np.uint32)     # one byte further
    first = np.array([TOK_MATCH | (3 << 16) | 11, ord("c")], np.uint32)                       # at position 0: D + 1
    lit = np.frombuffer(b"plain literals, then nothing", np.uint8).astype(np.uint32)
    streams = [DM.LM.stream(t) for t in (ok, bad, first, lit)]
    got, err = _decode(lib, dct, streams, [7, 7, 4, len(lit)], waves)
    assert err.tolist() == [0, errno.EINVAL, errno.EINVAL, 0]
    assert got[:7] == b"ab0123c" and got[18:] == bytes(lit.astype(np.uint8))
    # without a history the first stream is refused too: dist > position, as it always was
    got, err = _decode(lib, b"", streams, [7, 7, 4, len(lit)], waves)
    assert err.tolist() == [errno.EINVAL, errno.EINVAL, errno.EINVAL, 0]
