"""TEST INFRASTRUCTURE: an independent writer of SQZF VERSION-2 frames (include/sqz/sqz.h: stored blocks) -- Python
struct + zlib.crc32 + the CPU oracle per block, on top of tests/frame_writer.py -- the cases whose outcome the
oracle decided beforehand, and the malformed version-2 variants the refusal tests feed to the readers.  Nothing here
calls the product."""
import errno
import functools
import struct
import zlib

import numpy as np

import frame_writer as W
import oracle_lib as O

STORED = 1                 # flags bit 0
STORED_BIT = 1 << 31       # of an index entry's first word

# (name, corpus file or literal bytes, win_bits, block_bits, blocks, stored blocks, version-1 payload,
#  version-2 payload, version-2 frame): measured with the CPU oracle, the writer below must arrive at every figure
CASES = [
    ("mandrill_bmp_w15_b14", "mandrill.bmp", 15, 14, 49, 11, 773464, 773024, 773456),
    ("mandrill_bmp_w10_b18", "mandrill.bmp", 10, 18, 4, 1, 774776, 774752, 774816),
    ("x64_w15_b12", "x64.elf", 15, 12, 227, 1, 513408, 513176, 515032),
    ("mandrill_png_w15_b14", "mandrill.png", 15, 14, 39, 39, 646280, 627896, 628248),
    ("laozi_w15_b12", "laozi.txt", 15, 12, 6, 0, 10544, 10544, 10624),
    ("one_byte", b"a", 15, 18, 1, 1, 8, 8, 56),
    ("empty", b"", 15, 18, 0, 0, 0, 0, 32),
]
CASE_IDS = [c[0] for c in CASES]
MIXED = ("mandrill_bmp_w15_b14", "mandrill_bmp_w10_b18", "x64_w15_b12")      # at least one block of either kind
ALL_STORED = ("mandrill_png_w15_b14", "one_byte")


def pad8(n: int) -> int:
    return (n + 7) & ~7


def pad16(n: int) -> int:
    return (n + 15) & ~15


def assemble(data: bytes, win_bits: int, block_bits: int, streams) -> bytes:
    """the writer's rule: block b is stored iff its stream is not smaller than its content"""
    blocks = W.blocks_of(data, block_bits)
    assert len(blocks) == len(streams) and all(len(s) % 8 == 0 for s in streams)
    index, payload = b"", []
    for s, b in zip(streams, blocks):
        stored = len(s) >= len(b)
        share = b + bytes(-len(b) % 8) if stored else s
        index += struct.pack("<II", len(share) // 8 | (STORED_BIT if stored else 0), zlib.crc32(b))
        payload.append(share)
    head = struct.pack("<4sBBBBQQI", b"SQZF", 2, win_bits, block_bits, STORED, len(data),
                       sum(len(p) for p in payload), len(blocks))
    front = head + struct.pack("<I", zlib.crc32(head + index)) + index
    return front + bytes(-len(front) % 16) + b"".join(payload)


def streams_of(data: bytes, win_bits: int, block_bits: int, encode=None):
    if encode is None:
        encode = lambda blk: O.encode(blk, win_bits, header=False)
    return [encode(b) for b in W.blocks_of(data, block_bits)]


def write_frame(data: bytes, win_bits: int, block_bits: int, encode=None) -> bytes:
    return assemble(data, win_bits, block_bits, streams_of(data, win_bits, block_bits, encode))


def case(name: str):
    return next(c for c in CASES if c[0] == name)


def case_data(name: str) -> bytes:
    src = case(name)[1]
    return src if isinstance(src, bytes) else O.corpus(src)


@functools.lru_cache(maxsize=None)
def case_streams(name: str):
    _, _, wb, bits = case(name)[:4]
    return tuple(streams_of(case_data(name), wb, bits))


@functools.lru_cache(maxsize=None)
def case_frame(name: str) -> bytes:
    """the version-2 frame of a case, held against the table's figures (the writer's self-check)"""
    _, _, wb, bits, n, n_stored, v1_payload, v2_payload, v2_frame = case(name)
    data, streams = case_data(name), case_streams(name)
    frame = assemble(data, wb, bits, streams)
    blk = blocks(frame)
    assert len(blk) == n and sum(b["stored"] for b in blk) == n_stored, name
    assert sum(len(s) for s in streams) == v1_payload and sum(b["payload_bytes"] for b in blk) == v2_payload, name
    assert len(frame) == v2_frame == pad16(32 + 8 * n) + v2_payload, name
    if name in MIXED:
        assert 0 < n_stored < n
    if name in ALL_STORED:
        assert n_stored == n > 0
    return frame


@functools.lru_cache(maxsize=None)
def case_frame_v1(name: str) -> bytes:
    _, _, wb, bits = case(name)[:4]
    return W.assemble(case_data(name), wb, bits, list(case_streams(name)))


def random_bytes(n: int, seed: int = 7) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def fields(frame: bytes) -> dict:
    """the header as laid out (no checking): the keys of frame_writer.fields for either version"""
    return W.fields(frame)


def flags_of(frame: bytes) -> int:
    return frame[7]


def blocks(frame: bytes) -> list:
    """per block what the index says, for either version (no checking)"""
    f = W.fields(frame)
    out, at = [], f["payload_off"]
    for b in range(f["n_blocks"]):
        word, crc = struct.unpack_from("<II", frame, 32 + 8 * b)
        stored = f["version"] == 2 and (word & STORED_BIT) != 0
        words = word & ~STORED_BIT if f["version"] == 2 else word
        out.append({"payload_off": at, "payload_bytes": 8 * words,
                    "content_bytes": min(f["block_bytes"], f["content_bytes"] - b * f["block_bytes"]),
                    "content_crc": crc, "stored": int(stored)})
        at += 8 * words
    return out


def refusals(frame: bytes):
    """(name, malformed frame, errno from the header alone, errno with the index in reach): each a valid version-2
    frame with a stored and a stream block and ONE change"""
    f, blk = W.fields(frame), blocks(frame)
    assert f["version"] == 2 and flags_of(frame) == STORED
    s = next(b for b, x in enumerate(blk) if x["stored"])
    t = next(b for b, x in enumerate(blk) if not x["stored"])
    E = errno.EINVAL
    out = []

    def put(name, at, fmt, value, head_errno, full_errno, reseal=False):
        b = bytearray(frame)
        struct.pack_into(fmt, b, at, value)
        out.append((name, W.reseal(b) if reseal else bytes(b), head_errno, full_errno))

    put("v2_flags_0", 7, "<B", 0, E, E)
    put("v2_flags_2", 7, "<B", 2, E, E)
    put("v2_flags_3", 7, "<B", 3, E, E)
    put("v1_flags_1", 4, "<B", 1, E, E)
    word = struct.unpack_from("<I", frame, 32 + 8 * s)[0]
    put("stored_one_word_more", 32 + 8 * s, "<I", word + 1, 0, E, reseal=True)
    put("stored_one_word_less", 32 + 8 * s, "<I", word - 1, 0, E, reseal=True)
    word = struct.unpack_from("<I", frame, 32 + 8 * t)[0]
    put("stored_bit_flipped_stale_crc", 32 + 8 * t, "<I", word | STORED_BIT, 0, errno.EILSEQ)
    put("payload_bytes_plus_8", 16, "<Q", f["payload_bytes"] + 8, 0, E, reseal=True)
    put("payload_bytes_minus_8", 16, "<Q", f["payload_bytes"] - 8, 0, E, reseal=True)
    return out
