"""TEST INFRASTRUCTURE: the shared inputs of the update tests (test_frame_update_emu.py, test_frame_update_gpu.py):
the frames, patterns and range lists of tests/frame_gather_cases.py, a TARGET content per pattern that the ranges'
data is cut from, the patched content, and the frame the independent writers (tests/frame_writer*.py, oracle_lib,
dict_model) make of it.  Nothing here calls the product.

In the target block k carries the letter of its neighbour and the last block stays: noise lands where text was and the
other way round, so the stored bit of versions 2 and 3 flips both ways.  The data of range r is target[o : o + n], so
overlapping ranges agree wherever they overlap and the expected frame is unique whichever of them wins."""
import functools

import dict_model as DM
import frame_gather_cases as G
import frame_writer as W
import frame_writer_v2 as W2
import frame_writer_v3 as W3
import oracle_lib as O

WB, BITS, BB = G.WB, G.BITS, G.BB


def target_pattern(name: str) -> str:
    p = G.PATTERNS[name]
    n = len(p)
    return "".join(p[k + 1] if k + 1 <= n - 2 else p[k - 1] for k in range(n - 1)) + p[-1]


@functools.lru_cache(maxsize=None)
def target(name: str) -> bytes:
    return b"".join(G.piece(c) for c in target_pattern(name))


def data_of(name: str, offsets, lengths, cap: int) -> bytes:
    """the bytes of the valid ranges, packed in request order"""
    t = target(name)
    return b"".join(t[o:o + n] for o, n in zip(offsets, lengths) if G.valid(o, n, cap, len(t)))


def patched(name: str, offsets, lengths, cap: int) -> bytes:
    out, t = bytearray(G.content(name)), target(name)
    for o, n in zip(offsets, lengths):
        if G.valid(o, n, cap, len(t)):
            out[o:o + n] = t[o:o + n]
    return bytes(out)


@functools.lru_cache(maxsize=None)
def stream_of(block: bytes, version: int, lazy: bool) -> bytes:
    if version == 3:
        return DM.stream(G.dct(), block, 1 << WB, lazy)
    assert not lazy                                  # the C oracle is the greedy parse
    return O.encode(block, WB, header=False)


def frame_of(data: bytes, version: int, lazy: bool = False) -> bytes:
    """the independent writer's frame of `data` at this version"""
    streams = [stream_of(b, 1 if version == 2 else version, lazy) for b in W.blocks_of(data, BITS)]
    if version == 1:
        return W.assemble(data, WB, BITS, streams)
    if version == 2:
        return W2.assemble(data, WB, BITS, streams)
    return W3.assemble(data, WB, BITS, G.dct(), streams, store=True)


def check_layout():
    """what the inputs are there for"""
    assert target_pattern("mixed") == "NAS" and target_pattern("whole") == "NbNA" and target_pattern("short") == "NbNt"
    for name in G.PATTERNS:
        assert len(target(name)) == len(G.content(name))
        assert target_pattern(name)[-1] == G.PATTERNS[name][-1]
    # a whole-content write turns the frame into the target's: the stored bit flips both ways in versions 2 and 3
    for version in (2, 3):
        for name in ("mixed", "whole"):
            size = len(G.content(name))
            assert patched(name, [0], [size], size) == target(name)
            old = [e["stored"] for e in G.block_entries(G.frame(name, version), version)]
            new = [e["stored"] for e in G.block_entries(frame_of(target(name), version), version)]
            assert any(a and not b for a, b in zip(old, new)) and any(b and not a for a, b in zip(old, new))
    assert frame_of(G.content("mixed"), 1) == G.frame("mixed", 1) and frame_of(G.content("short"), 2) == G.frame("short", 2)
