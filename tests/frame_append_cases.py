"""TEST INFRASTRUCTURE: the shared inputs of the append tests (test_frame_append_emu.py, test_frame_append_gpu.py):
old contents (the frames of tests/frame_gather_cases.py, the empty content and two whose ragged last block is there for
the stored bit), a supply of data to put behind each, the lengths to cut from it, and the frame the independent writers
(tests/frame_writer*.py, oracle_lib, dict_model) make of old + data.  Nothing here calls the product.

The lengths go around fill = the bytes that complete a ragged last block: the new frame then ends in the touched block,
exactly on its edge, one byte behind it (a 1-byte block, which is always stored), and one, one and a bit, and three
blocks further, so that n' is odd and even both ways, with and without the dictionary's record."""
import functools

import frame_gather_cases as G
import frame_update_cases as U
import frame_v3_cases as K
import frame_writer_v2 as W2

WB, BITS, BB = G.WB, G.BITS, G.BB
frame_of = U.frame_of


@functools.lru_cache(maxsize=None)
def old_content(name: str) -> bytes:
    if name in G.PATTERNS:
        return G.content(name)
    return {"empty": b"",
            "noise_tail": G.piece("a") + G.piece("N")[:904],         # a stored ragged block that text completes
            "tiny_text_tail": G.piece("a") + G.piece("t")[:100]}[name]   # 100 compressible bytes that noise completes


OLD = ("short", "whole", "mixed", "b70", "b300", "empty", "noise_tail", "tiny_text_tail")


@functools.lru_cache(maxsize=None)
def cheap(n_blocks: int) -> bytes:
    """a run of the pieces a .. p: blocks of a few tokens each (the wave emulator's time goes with the tokens)"""
    return b"".join(G.piece("abcdefghijklmnop"[k % 16]) for k in range(n_blocks))


@functools.lru_cache(maxsize=None)
def supply(kind: str) -> bytes:
    noise = W2.random_bytes(8192, 12)
    base = {"noise": noise,
            "text": K.lao()[8000:8000 + 8192],
            "mix": noise[:2048] + G.piece("c") + G.piece("A") + noise[2048:6144] + G.piece("d"),
            "cheap": b""}[kind]
    return base + cheap(192)                                 # behind 8 KB of noise or text: cheap blocks


# what is put behind which old content: the other kind than its last block, so that the stored bit can flip
KIND = {"short": "mix", "whole": "text", "mixed": "noise", "b70": "cheap", "b300": "cheap", "empty": "mix",
        "noise_tail": "text", "tiny_text_tail": "noise"}


def tail_bytes(name: str) -> int:
    return len(old_content(name)) % BB


def fill(name: str) -> int:
    return (BB - tail_bytes(name)) % BB


def lengths(name: str):
    f = fill(name)
    out = []
    for n in (0, 1, f - 1, f, f + 1, f + BB, f + BB + 904, f + 3 * BB + 1):
        if n >= 0 and n not in out:
            out.append(n)
    return out


def data_of(name: str, length: int) -> bytes:
    d = supply(KIND[name])[:length]
    assert len(d) == length
    return d


def shape(name: str, length: int):
    """(t, touched, keep, m, n') by the call's arithmetic"""
    size = len(old_content(name))
    n, t = (size + BB - 1) // BB, size % BB
    touched = t > 0 and length > 0
    keep = n - (1 if touched else 0)
    m = ((t if touched else 0) + length + BB - 1) // BB if length > 0 else 0
    return t, touched, keep, m, keep + m


def cases():
    """(old content's name, data length) for every old content, and the two long appends"""
    out = [(name, n) for name in OLD for n in lengths(name)]
    out.append(("b70", fill("b70") + 190 * BB))              # 69 + 191 = 260 blocks: lanes with two entries and with none
    return out


def expected(name: str, length: int, version: int, lazy: bool = False) -> bytes:
    return frame_of(old_content(name) + data_of(name, length), version, lazy)


def old_frame(name: str, version: int, lazy: bool = False) -> bytes:
    return frame_of(old_content(name), version, lazy)


def stored_bits(frame: bytes, version: int) -> str:
    return "".join("S" if e["stored"] else "." for e in G.block_entries(frame, version))


def check_layout():
    """what the inputs are there for"""
    assert [tail_bytes(k) for k in OLD] == [904, 0, 904, 904, 904, 0, 904, 100]
    assert fill("noise_tail") == 3192 and fill("tiny_text_tail") == 3996 and fill("short") == 3192 and fill("whole") == 0
    for v in (1, 2, 3):
        assert old_frame("short", v) == G.frame("short", v) and old_frame("b70", v) == G.frame("b70", v)
        assert len(old_frame("empty", v)) == (48 if v == 3 else 32)
    for v in (2, 3):
        # the touched block stops being stored, becomes stored, and a 1-byte block behind it is stored
        assert stored_bits(old_frame("noise_tail", v), v) == ".S" and stored_bits(expected("noise_tail", 3192, v), v) == ".."
        assert stored_bits(old_frame("tiny_text_tail", v), v) == ".." and stored_bits(expected("tiny_text_tail", 3996, v), v) == ".S"
        assert stored_bits(old_frame("short", v), v) == ".S.." and stored_bits(expected("short", 3193, v), v) == ".S..S"
    assert [len(old_frame("noise_tail", 1)), len(expected("noise_tail", 3192, 1))] == [1104, 2856]
    assert [len(old_frame("tiny_text_tail", 1)), len(expected("tiny_text_tail", 3996, 1))] == [104, 4320]
    # n' through every value the padding and the scans need
    news = {(name, n): shape(name, n)[4] for name, n in cases()}
    olds = {name: (len(old_content(name)) + BB - 1) // BB for name in OLD}
    flips = {(olds[name] % 2, n_new % 2) for (name, _), n_new in news.items()}
    assert flips == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {news[("empty", n)] for n in lengths("empty")} >= {0, 1, 2}
    assert news[("b70", fill("b70") + 190 * BB)] == 260 and news[("b300", fill("b300") + BB)] == 301
    assert all(shape(name, 0)[1:] == (False, olds[name], 0, olds[name]) for name in OLD)
