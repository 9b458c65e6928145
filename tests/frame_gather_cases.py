"""TEST INFRASTRUCTURE: the shared inputs of the gather tests (test_frame_gather_emu.py, test_frame_gather_gpu.py):
frames of 4 KB blocks from the independent writers (tests/frame_writer*.py, tests/dict_model.py), lists of byte
ranges, and a few lines of Python over the plain content that say what a gather of them delivers.  Nothing here
calls the product.  Blocks are independent, so a long frame is a pattern over four distinct 4 KB contents whose
streams are computed once per version."""
import errno
import functools
import random

import dict_model as DM
import frame_v3_cases as K
import frame_writer as W
import frame_writer_v2 as W2
import frame_writer_v3 as W3
import oracle_lib as O

WB, BITS = 15, 12
BB = 1 << BITS
M64 = (1 << 64) - 1
EDGES = (31, 32, 33, 63, 64, 65, 255, 256, 257, 299)

# a pattern is one letter per block: A a block of text, N a block of noise (stored in versions 2 and 3), S a short block
# of text (904 bytes), a .. p sixteen different blocks that compress to a few tokens (the wave emulator's time goes with
# the tokens: the long frames are made of these), t a short one (904 bytes).  S and t can only be the last block.
def _long(n: int, noise_every: int, text_at: int) -> str:
    cells = ["N" if k % noise_every == noise_every - 1 else "abcdefghijklmnop"[k % 16] for k in range(n - 1)]
    cells[text_at] = "A"
    return "".join(cells) + "t"


PATTERNS = {
    "mixed": "ANS",                                  # frame_v3_cases.mixed(): three blocks, the middle one stored
    "whole": "aNbA",                                 # the content ends on a block edge
    "short": "aNbt",                                 # a short last block
    "b70": _long(70, 3, 33),                         # 70 blocks: bitmap word edges at 31/32/33 and 63/64/65
    "b300": _long(300, 5, 256),                      # 300 blocks: more than one index entry per thread of 256
}


@functools.lru_cache(maxsize=None)
def piece(letter: str) -> bytes:
    lao = K.lao()
    if letter in "abcdefghijklmnopt":
        k = ord(letter) - ord("a")
        return (bytes((k * 37 + j * (11 + k)) % 251 for j in range(8 + k % 5)) * 512)[:904 if letter == "t" else 4096]
    return {"A": lao[3000:7096], "N": W2.random_bytes(4096, 11), "S": lao[7096:8000]}[letter]


def dct() -> bytes:
    return K.dct()


@functools.lru_cache(maxsize=None)
def content(name: str) -> bytes:
    return b"".join(piece(c) for c in PATTERNS[name])


@functools.lru_cache(maxsize=None)
def _stream(letter: str, version: int, lazy: bool) -> bytes:
    if version == 3:
        return DM.stream(dct(), piece(letter), 1 << WB, lazy)
    return O.encode(piece(letter), WB, header=False)


@functools.lru_cache(maxsize=None)
def frame(name: str, version: int, lazy: bool = False) -> bytes:
    data = content(name)
    streams = [_stream(c, version, lazy) for c in PATTERNS[name]]
    if version == 1:
        return W.assemble(data, WB, BITS, streams)
    if version == 2:
        return W2.assemble(data, WB, BITS, streams)
    return W3.assemble(data, WB, BITS, dct(), streams, store=True)


def block_entries(frame_bytes: bytes, version: int):
    return W3.blocks(frame_bytes) if version == 3 else W2.blocks(frame_bytes)


def covering(offset: int, length: int):
    return range(offset >> BITS, ((offset + length - 1) >> BITS) + 1) if length > 0 else range(0)


def valid(offset: int, length: int, max_length: int, size: int) -> bool:
    return length <= max_length and offset <= size and length <= size - offset


def model(data: bytes, offsets, lengths, max_length: int, bad_blocks=(), bad_errno=errno.EILSEQ):
    """(out, out_off, range_err, distinct covering blocks in ascending order, [delivered?]) of a gather that succeeds;
    bad_blocks: blocks that fail (their ranges carry bad_errno and are not delivered: out has None there)"""
    out_off, range_err, blocks, parts = [0], [], set(), []
    for o, n in zip(offsets, lengths):
        ok = valid(o, n, max_length, len(data))
        hit = ok and any(b in bad_blocks for b in covering(o, n))
        range_err.append(errno.EINVAL if not ok else bad_errno if hit else 0)
        parts.append(None if not ok or hit else data[o:o + n])
        if ok:
            blocks.update(covering(o, n))
        out_off.append(out_off[-1] + (n if ok else 0))
    return parts, out_off, range_err, sorted(blocks)


def many(name: str, count: int, seed: int, most: int = 300):
    """`count` ranges at random offsets, odd and even lengths 0..most (one of them 0), none invalid"""
    size, rng = len(content(name)), random.Random(seed)
    lengths = [rng.randrange(0, most + 1) for _ in range(count)]
    lengths[count // 2] = 0
    return [rng.randrange(0, size - n + 1) for n in lengths], lengths, most


@functools.lru_cache(maxsize=None)
def range_lists(name: str):
    """{list name: (offsets, lengths, max_length)} for the content `name`"""
    size = len(content(name))
    n = len(PATTERNS[name])
    last = (n - 1) * BB
    out = {
        "one": ([4090], [12], 12),
        "zero": ([100, size, 0], [0, 0, 0], 0),
        "to_the_end": ([size - 50], [50], 64),
        "one_edge": ([4090], [12], 4096),
        "two_edges": ([4000], [4300], 4300),
        "last_block": ([last + 3], [size - last - 5], 4096),
        "two_in_one_block": ([10, 200], [20, 30], 30),
        "twice": ([4090, 4090], [12, 12], 12),
        "descending": ([8200, 4100, 5], [100, 50, 7], 100),
        "invalid": ([5, size + 1, 9, M64 - 1, 20, 30, 40], [7, 0, 3, 5, 4, 51, 2], 50),
        "unaligned": ([1, 4099, 8191, 77, 4093, 6], [3, 17, 33, 1, 4099, 15], 4099),
        "whole": ([0], [size], size),
    }
    for count in (63, 64, 65, 255, 256, 257):
        out[f"many_{count}"] = many(name, count, count)
    edges = [b for b in EDGES if b < n]
    if edges:                                        # the long frames: single blocks at the bitmap's word edges, and a
        offs = [b * BB + 100 + b for b in edges] + [32 * BB - 5, 64 * BB - 3]     # range across each of the first two
        out["word_edges"] = (offs, [41] * len(edges) + [10, 7], 41)
    return out


def check_layout():
    """what the inputs are there for, asserted from the writers and the lists themselves"""
    assert content("mixed") == K.mixed()
    for v, want in ((1, [0, 0, 0]), (2, [0, 1, 0]), (3, [0, 1, 0])):
        assert [b["stored"] for b in block_entries(frame("mixed", v), v)] == want
        assert W2.fields(frame("mixed", v))["version"] == v
    assert [len(PATTERNS[k]) for k in ("b70", "b300")] == [70, 300]
    assert len(content("whole")) % BB == 0 and len(content("short")) % BB == 904 and len(content("b300")) % BB == 904
    assert PATTERNS["b70"][31:34] == "pNA" and PATTERNS["b300"][255:258] == "pAb" and PATTERNS["b300"][299] == "t"
    for v in (2, 3):                                 # the noise is stored, nothing else is
        assert all(e["stored"] == (c == "N") for e, c in zip(block_entries(frame("b70", v), v), PATTERNS["b70"]))
    for name in PATTERNS:
        size, n = len(content(name)), len(PATTERNS[name])
        L = range_lists(name)
        cov = lambda key, k=0: list(covering(L[key][0][k], L[key][1][k]))
        assert cov("one") == [0, 1] and cov("one_edge") == [0, 1] and cov("two_edges") == [0, 1, 2]
        assert all(not list(covering(o, n_)) and valid(o, n_, 0, size) for o, n_ in zip(*L["zero"][:2]))
        assert L["to_the_end"][0][0] + L["to_the_end"][1][0] == size
        assert cov("last_block") == [n - 1] and L["last_block"][1][0] > 0
        assert cov("two_in_one_block", 0) == cov("two_in_one_block", 1) == [0]
        assert L["twice"][0][0] == L["twice"][0][1]
        assert L["descending"][0] == sorted(L["descending"][0], reverse=True)
        o, ln, cap = L["invalid"]
        assert [valid(a, b, cap, size) for a, b in zip(o, ln)] == [True, False, True, False, True, False, True]
        assert o[1] > size and (o[3] + ln[3]) >> 64 == 1 and ln[5] > cap      # one invalid range of each kind
        o, ln, cap = L["unaligned"]
        assert all(x % 2 == 1 for x in ln) and any(a % 16 != 0 for a in o)
        for count in (63, 64, 65, 255, 256, 257):
            o, ln, cap = L[f"many_{count}"]
            assert len(o) == count and all(valid(a, b, cap, size) for a, b in zip(o, ln)) and 0 in ln
    for name, want in (("b70", EDGES[:6]), ("b300", EDGES)):
        o, ln, cap = range_lists(name)["word_edges"]
        assert sorted(set().union(*(covering(a, b) for a, b in zip(o, ln)))) == list(want)
    assert "word_edges" not in range_lists("mixed")
