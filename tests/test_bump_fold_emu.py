"""CPU: the batched tree update (sqz_amd/csrc/sqz_tree.h: bump_batch) after two changes that must not move a
bit of any stream, on the CPU wave emulator (tests/emu, built as tests/test_emu.py builds it, all four variants):

  * the distance tree's internal nodes are probed in lanes 32-63 of the literal tree's fifth row (the literal
    tree's ids kRoot + 256 .. kRoot + 287 take lanes 0-31 of it) instead of in a row of their own;
  * an offer ends in front of the first token whose own leaf has no slack (it has a test partner whose count
    does not exceed the leaf's), before anything is counted.

Every case is held against the oracle byte for byte, and the one-wave and the 4-wave decoder give the input
back.  What a case is FOR (a literal node allocated in the shared row, a cut at lane 0, ...) is asserted too,
from the one line per call that the emulator's -DSQZ_EMU_DEBUG_BATCH build prints: a case that does not reach
its condition proves nothing.

The case "the leaf is the root's only child" cannot be given to the emit kernel as tokens: the only leaf that
is ever alone under a root is the escape symbol's, and no token word names it (token_ok).  The hi child of a
root is the same code path (partner kNil, the clamped read returns the leaf's own count) and is what 2(d)
drives through the emit kernel; the root's only child itself is driven through emu_tree_debug (test 3b).

Same cuts: the debug build of the parent's sources (git) and of this tree take the same steps, apply and
settle the same tokens one at a time, and this tree counts fewer offered tokens
(test_same_steps_fewer_offered_tokens has the figures)."""
import ctypes as C
import os
import random
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import oracle_lib as O
import test_emu as TE

ROOT = TE.ROOT
MATCH = 0x80000000
LIT_ROOT, POS_ROOT = 288, 576 + 32            # node ids of the two roots (sqz_tree.h: kLitLeaves, kPosBase + kPosLeaves)


def M(length, dist):
    return MATCH | (length << 16) | dist


def len_sym(length):
    y = length - 3
    if y < 8:
        return y
    msb = y.bit_length() - 1
    return 4 * msb - 4 + ((y >> (msb - 2)) & 3)


def pos_sym(dist):
    if dist < 5:
        return dist - 1
    x = dist - 1
    msb = x.bit_length() - 1
    return 2 * msb + ((x >> (msb - 1)) & 1)


def expand(tokens):
    out = bytearray()
    for t in tokens:
        t = int(t)
        if t & MATCH:
            ln, d = (t >> 16) & 0x1FF, t & 0x7FFF
            assert 1 <= d <= len(out)
            for _ in range(ln):
                out.append(out[-d])
        else:
            out.append(t)
    return bytes(out)


# ---- the debug build: one "batch ..." line per call of bump_batch, totals per stream ---------------------
def _debug_lib(src_root, out, flags=()):
    emu = os.path.join(src_root, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-DSQZ_EMU_DEBUG_BATCH", *flags, "-I" + emu,
                           "-I" + os.path.join(src_root, "include"), "-Wno-unused-function", "-Wno-unused-variable",
                           "-Wno-attributes", os.path.join(emu, "emu_runtime.cpp"), os.path.join(emu, "emu_emit.cpp"),
                           "-o", out])
    return C.CDLL(out)


def _parent_rev():
    """the commit in front of the one that brought the cut (HEAD itself while that one is not committed yet)"""
    git = ["git", "-C", ROOT]
    try:
        r = subprocess.run(git + ["log", "--format=%H", "-S", "SQZ_BATCH_NO_CUT", "--", "sqz_amd/csrc/sqz_tree.h"],
                           capture_output=True, text=True)
        if r.returncode != 0:
            return None
        revs = r.stdout.split()
        rev = revs[-1] + "~" if revs else "HEAD"
        ok = subprocess.run(git + ["cat-file", "-e", rev + ":sqz_amd/csrc/sqz_tree.h"], capture_output=True).returncode == 0
        return rev if ok else None
    except OSError:
        return None


@pytest.fixture(scope="module")
def debug_libs(tmp_path_factory):
    """(this tree's debug build, the baseline's, what the baseline is)"""
    tmp = str(tmp_path_factory.mktemp("bump_fold"))
    new = _debug_lib(ROOT, os.path.join(tmp, "libdbg_new.so"))
    rev = _parent_rev()
    if rev is not None:
        src = os.path.join(tmp, "parent")
        os.makedirs(src)
        ar = subprocess.Popen(["git", "-C", ROOT, "archive", rev, "tests/emu", "sqz_amd/csrc", "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", src], stdin=ar.stdout)
        assert ar.wait() == 0
        return new, _debug_lib(src, os.path.join(tmp, "libdbg_parent.so")), "parent sources " + rev
    # no history to take the parent from: this tree with the cut compiled out offers what the parent offered
    return new, _debug_lib(ROOT, os.path.join(tmp, "libdbg_nocut.so"), ["-DSQZ_BATCH_NO_CUT"]), "this tree, -DSQZ_BATCH_NO_CUT"


def traced_emit(E, tokens):
    """-> (stream, the debug build's stderr lines)"""
    tokens = np.asarray(tokens, np.uint32)
    with tempfile.TemporaryFile() as tf:
        sys.stderr.flush()
        keep = os.dup(2)
        os.dup2(tf.fileno(), 2)
        try:
            outs, err = TE.emit(E, [tokens], [max(len(tokens), 1)])
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tf.seek(0)
        lines = tf.read().decode().splitlines()
    assert err.tolist() == [0]
    return outs[0], lines


_BATCH = re.compile(r"batch m (\d+) cut (-?\d+) a (\w+) b (\w+) nil (\w+) bad((?: \w+)+) ok (\d+) next (\d+) (\d+)")


def batches(lines):
    out = []
    for l in lines:
        g = _BATCH.match(l)
        if g:
            out.append(dict(m=int(g[1]), cut=int(g[2]), a=int(g[3], 16), b=int(g[4], 16), nil=int(g[5], 16),
                            bad=[int(x, 16) for x in g[6].split()], ok=int(g[7]), lit_inner=int(g[8]), pos_inner=int(g[9])))
    return out


def totals(lines):
    t = dict(steps=0, offered=0, applied=0, exact=0)
    for l in lines:
        g = re.match(r"cursor \d+: steps (\d+) offered (\d+) applied (\d+) exact (\d+)", l)
        if g:
            for k, v in zip(("steps", "offered", "applied", "exact"), g.groups()):
                t[k] += int(v)
    return t


def lanes(mask):
    return [k for k in range(64) if (mask >> k) & 1]


# what each token case is for, as a predicate over one call's line
def hits_a(c):
    return c["cut"] == 0 and c["ok"] == 0


def hits_b(c):
    return c["m"] >= 4 and c["cut"] == c["m"] - 1


def hits_c(c):
    la, lb = lanes(c["a"]), lanes(c["b"])
    return bool(la) and bool(lb) and c["cut"] == min(la + lb) and any(x != y for x in la for y in lb)


def hits_d(c):
    # a leaf without a test partner offered in every lane: nothing cuts, nothing fails, everything is applied
    return c["m"] >= 16 and c["nil"] == (1 << c["m"]) - 1 and c["cut"] == -1 and c["ok"] == c["m"]


def hits_e(c):
    # a leaf's own test fails in front of the cut, in two lanes at least (the leaf was met twice and had some
    # slack, or the cut would have been there): located, and the prefix counted again
    below = (1 << max(c["cut"], 0)) - 1
    leaf = (c["bad"][0] | c["bad"][1]) & below
    return c["cut"] >= 3 and bin(leaf).count("1") >= 2 and 0 < c["ok"] < c["cut"]


def hits_f(c):
    shared = c["bad"][-1]
    return (shared & 0xFFFFFFFF) != 0 and (shared >> 32) != 0


def mixed_tokens(seed, full=False):
    """tokens over a small alphabet (full: behind all 256 byte values, so that the literal tree's last inserts
    land in the shared row), distances never further back than what has been produced"""
    rng = random.Random(seed)
    toks, made = [], 0

    def lit(v):
        nonlocal made
        toks.append(v)
        made += 1

    def match():
        nonlocal made
        d = rng.choice([x for x in dists if x <= made] or [1])
        ln = rng.choice(lens)
        toks.append(M(ln, d))
        made += ln

    if full:
        for v in range(256):
            lit(v)
        lens = rng.sample([3, 4, 5, 6, 9, 12, 20, 40, 100], 5)
        dists = rng.sample([1, 2, 3, 4, 6, 9, 14, 20, 40, 70, 130, 300, 600, 1500], 9)
        for _ in range(rng.randrange(300, 700)):
            if rng.random() < 0.5:
                match()
            else:
                lit(rng.randrange(256) if rng.random() < 0.2 else rng.choice([7, 9, 200]))
    else:
        lits = rng.sample(range(256), rng.randrange(3, 9))
        lens = rng.sample([3, 4, 5, 9, 12, 20, 40, 100], rng.randrange(1, 4))
        dists = rng.sample([1, 2, 3, 4, 6, 9, 14, 20, 40, 70, 130, 300], rng.randrange(2, 6))
        weight = [rng.random() ** 2 for _ in lits]
        lit(lits[0])
        for _ in range(rng.randrange(150, 400)):
            if rng.random() < 0.35:
                match()
            else:
                lit(rng.choices(lits, weight)[0])
    return toks


TOKEN_CASES = {
    "a_no_slack_leaf_in_lane_0": (mixed_tokens(0), hits_a),
    "b_no_slack_leaf_in_the_last_offered_lane": (mixed_tokens(6), hits_b),
    "c_no_slack_leaves_on_both_sides_of_different_tokens": (mixed_tokens(1), hits_c),
    "d_leaf_without_a_test_partner": ([65] * 40 + [66] + [65] * 300 + [66, 67] + [65] * 100, hits_d),
    "e_slack_used_up_in_front_of_the_cut": (mixed_tokens(4), hits_e),
    "f_both_halves_of_the_shared_row_fail": (mixed_tokens(0, full=True), hits_f),
}


def shared_row_block():
    """6 KB: every byte value once, then repeats of many lengths from many distances"""
    rng = random.Random(5)
    out = bytearray(range(256))
    while len(out) < 6144:
        d = rng.choice([1, 2, 3, 4, 6, 10, 20, 40, 90, 200, 500, 1500, 3000])
        ln = rng.choice([3, 4, 5, 8, 13, 30, 70])
        if d <= len(out):
            for _ in range(ln):
                out.append(out[-d])
        out.append(rng.randrange(256))
    return bytes(out)


def _oracle(name):
    """(encode bytes, encode tokens) of the oracle that belongs to a build: the freeze build has one with its threshold"""
    L = O.ORACLE
    if name == "freeze":
        subprocess.check_call(["make", "-C", O.ODIR, "-s", "freeze9"])
        L = C.CDLL(os.path.join(O.ODIR, "liboracle_freeze9.so"))
        L.sqzo_encode.restype = C.c_int
        L.sqzo_encode.argtypes = O.ORACLE.sqzo_encode.argtypes

    def enc(data, w):
        out = C.create_string_buffer(2 * len(data) + 1088)
        n = C.c_uint64()
        assert L.sqzo_encode(data, len(data), w, 0, out, len(out), C.byref(n)) == 0
        return out.raw[:n.value]

    def enc_tokens(tokens):
        toks = np.ascontiguousarray(tokens, dtype=np.uint32)
        out = C.create_string_buffer(8 * len(toks) + 64)
        n, st = C.c_uint64(0), O.Stats()
        assert L.sqzo_encode_tokens(TE._p(toks), C.c_uint64(len(toks)), out, C.c_uint64(len(out)), C.byref(n), C.byref(st)) == 0
        return out.raw[:n.value]
    return enc, enc_tokens


@pytest.fixture(scope="module", params=list(TE.VARIANTS))
def emu(request):
    name = request.param
    return (name, TE._build(name, "emit"), TE._build(name, "decode")) + _oracle(name)


def _round_trip(D, stream, data):
    for waves in (1, 4):
        back, derr = TE.decode(D, [stream], [len(data)], waves=waves)
        assert derr.tolist() == [0], waves
        assert back == [data], waves


def test_literal_node_in_the_shared_row_next_to_distance_nodes(emu, debug_libs):
    name, E, D, enc, _ = emu
    data = shared_row_block()
    assert 4096 <= len(data) <= 8192
    w = 1 << 12
    toks = O.tokens(data, w)
    m = [int(t) for t in toks if int(t) & MATCH]
    assert len({len_sym((t >> 16) & 0x1FF) for t in m}) >= 3 and len({pos_sym(t & 0x7FFF) for t in m}) >= 8
    want = enc(data, w)
    outs, err = TE.emit(E, [toks], [len(data)])
    assert err.tolist() == [0] and outs[0] == want
    _round_trip(D, want, data)
    if name == "default":
        # the literal tree's symbol sequence through the tree entry: its next free id lies in the shared row
        syms = np.array([257 + len_sym((int(t) >> 16) & 0x1FF) if int(t) & MATCH else int(t) for t in toks], np.int32)
        dump = np.zeros(8 + 4 * 576, np.uint32)
        E.emu_tree_debug(TE._p(syms), len(syms), 0, 64, TE._p(dump))
        assert int(dump[0]) > LIT_ROOT + 256, int(dump[0])
        # ... and batches ran with live nodes in both halves of that row
        stream, lines = traced_emit(debug_libs[0], toks)
        assert stream == outs[0]
        assert any(c["lit_inner"] > 256 and c["pos_inner"] > 8 and c["ok"] > 0 for c in batches(lines))


@pytest.mark.parametrize("case", list(TOKEN_CASES))
def test_token_cases(emu, debug_libs, case):
    name, E, D, _, enc_tokens = emu
    toks, hits = TOKEN_CASES[case]
    want = enc_tokens(toks)
    outs, err = TE.emit(E, [np.asarray(toks, np.uint32)], [len(toks)])
    assert err.tolist() == [0] and outs[0] == want
    _round_trip(D, want, expand(toks))
    if name == "default":
        stream, lines = traced_emit(debug_libs[0], toks)
        assert stream == want
        assert any(hits(c) for c in batches(lines)), "the case does not reach what it is for"


@pytest.mark.parametrize("batch", [1, 7, 64])
def test_reference_tree_fixtures(batch):
    """tests/golden/trees.npz, both trees: the dump equals the reference's node arrays, as tests/test_gpu_tree.py
    checks on the device"""
    import test_gpu_tree as T
    E = TE._build("default", "emit")
    z = np.load(os.path.join(O.GOLD, "trees.npz"))
    names = sorted({k.split(".")[0] for k in z.files})
    assert {int(z[n + ".n"]) for n in names} >= {512, 32}
    for name in names:
        n = int(z[name + ".n"])
        syms = z[name + ".symbols"][:2500]            # (the emulator makes ~5,000 updates a second)
        if n == 8:
            n = 32
        arrs, info = O.tree_run(O.ORACLE, "sqzo_tree_run", n, syms)
        which = 0 if n == 512 else 1
        nodes = 576 if which == 0 else 64
        s = np.ascontiguousarray(syms, dtype=np.int32)
        dump = np.zeros(8 + 4 * nodes, np.uint32)
        E.emu_tree_debug(TE._p(s), len(s), which, batch, TE._p(dump))
        T.compare(which, dump[:8], dump[8:].reshape(nodes, 4), n, arrs, info, T.oracle_counters(n, syms))


@pytest.mark.parametrize("which,sym", [(0, 285), (1, 30)])
def test_the_roots_only_child_is_not_cut(which, sym):
    """the escape symbol alone under its root (partner kNil), 200 times: the tree equals the oracle's"""
    import test_gpu_tree as T
    E = TE._build("default", "emit")
    n = 512 if which == 0 else 32
    nodes = 576 if which == 0 else 64
    syms = np.full(200, sym, np.int32)
    arrs, info = O.tree_run(O.ORACLE, "sqzo_tree_run", n, syms)
    dump = np.zeros(8 + 4 * nodes, np.uint32)
    E.emu_tree_debug(TE._p(syms), len(syms), which, 64, TE._p(dump))
    T.compare(which, dump[:8], dump[8:].reshape(nodes, 4), n, arrs, info, T.oracle_counters(n, syms))


def test_same_steps_fewer_offered_tokens(debug_libs):
    """steps, applied and exact are the parent's; offered is lower.  Measured (parent -> this tree):
         zipf block 1, 65536 bytes   3,038 steps, 53,840 applied, 2,246 exact; offered 86,997 -> 69,305
         laozi.txt[:9000]              664 steps,  2,558 applied,   585 exact; offered  6,832 ->  4,287"""
    new, base, what = debug_libs
    for data in (O.zipf_block(1, 65536), O.corpus("laozi.txt")[:9000]):
        toks = O.tokens(data, 1 << 12)
        s_new, l_new = traced_emit(new, toks)
        s_base, l_base = traced_emit(base, toks)
        assert s_new == s_base == O.encode(data, 12, header=False)
        t_new, t_base = totals(l_new), totals(l_base)
        print(what, len(data), "baseline", t_base, "new", t_new)
        assert t_new["steps"] > 0
        for k in ("steps", "applied", "exact"):
            assert t_new[k] == t_base[k], (k, t_new, t_base)
        assert t_new["offered"] < t_base["offered"], (t_new, t_base)
