"""TEST INFRASTRUCTURE: an independent writer of SQZF VERSION-3 frames (include/sqz/sqz.h: a shared dictionary) --
Python struct + zlib.crc32 + tests/dict_model.py per block.  Nothing here calls the product.

Version 3 = version 2's layout, flags bit 1 (DICT), and one 8-byte record { dict_bytes, dict_crc } directly behind
the n index entries, covered by index_crc; payload_off = pad16(32 + 8n + 8).  Bit 0 (STORED) may accompany bit 1."""
import struct
import zlib

import dict_model as DM
import frame_writer as W

STORED = 1                 # flags bit 0
DICT = 2                   # flags bit 1
STORED_BIT = 1 << 31       # of an index entry's first word


def pad16(n: int) -> int:
    return (n + 15) & ~15


def streams_of(data: bytes, win_bits: int, block_bits: int, dct: bytes, lazy: bool = False):
    return [DM.stream(dct, b, 1 << win_bits, lazy) for b in W.blocks_of(data, block_bits)]


def assemble(data: bytes, win_bits: int, block_bits: int, dct: bytes, streams, store: bool = False) -> bytes:
    blocks = W.blocks_of(data, block_bits)
    assert len(blocks) == len(streams) and all(len(s) % 8 == 0 for s in streams)
    index, payload = b"", []
    for s, b in zip(streams, blocks):
        stored = store and len(s) >= len(b)                 # the writer's rule of version 2, unchanged
        share = b + bytes(-len(b) % 8) if stored else s
        index += struct.pack("<II", len(share) // 8 | (STORED_BIT if stored else 0), zlib.crc32(b))
        payload.append(share)
    record = struct.pack("<II", len(dct), zlib.crc32(dct))
    head = struct.pack("<4sBBBBQQI", b"SQZF", 3, win_bits, block_bits, DICT | (STORED if store else 0), len(data),
                       sum(len(p) for p in payload), len(blocks))
    front = head + struct.pack("<I", zlib.crc32(head + index + record)) + index + record
    return front + bytes(-len(front) % 16) + b"".join(payload)


def write_frame(data: bytes, win_bits: int, block_bits: int, dct: bytes, store: bool = False, lazy: bool = False) -> bytes:
    return assemble(data, win_bits, block_bits, dct, streams_of(data, win_bits, block_bits, dct, lazy), store)


def fields(frame: bytes) -> dict:
    """the header and the record as laid out (no checking)"""
    magic, ver, wb, bits, flags, content, payload, n, crc = struct.unpack("<4sBBBBQQII", frame[:32])
    off = pad16(32 + 8 * n + 8)
    nb, dcrc = struct.unpack_from("<II", frame, 32 + 8 * n)
    return {"content_bytes": content, "payload_bytes": payload, "payload_off": off, "frame_bytes": off + payload,
            "block_bytes": 1 << bits, "n_blocks": n, "win_bits": wb, "version": ver, "dict_bytes": nb, "dict_crc": dcrc}


def blocks(frame: bytes) -> list:
    f = fields(frame)
    out, at = [], f["payload_off"]
    for b in range(f["n_blocks"]):
        word, crc = struct.unpack_from("<II", frame, 32 + 8 * b)
        share = 8 * (word & ~STORED_BIT)
        lo = b * f["block_bytes"]
        out.append({"payload_off": at, "payload_bytes": share,
                    "content_bytes": min(f["block_bytes"], f["content_bytes"] - lo), "content_crc": crc,
                    "stored": word >> 31})
        at += share
    return out


def reseal(frame: bytearray) -> bytes:
    """recompute index_crc over whatever header, index and record now say"""
    n = struct.unpack_from("<I", frame, 24)[0]
    struct.pack_into("<I", frame, 28, zlib.crc32(bytes(frame[:28]) + bytes(frame[32:32 + 8 * n + 8])))
    return bytes(frame)
