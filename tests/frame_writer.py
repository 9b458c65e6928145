"""TEST INFRASTRUCTURE: an independent writer of SQZF frames (include/sqz/sqz.h) -- Python struct + zlib.crc32 +
the CPU oracle per block -- and the malformed variants the refusal tests feed to the readers.  Nothing here
calls the product."""
import errno
import functools
import struct
import zlib

import oracle_lib as O

# (name, corpus file or literal bytes, win_bits, block_bits, frame size the writer must arrive at)
CASES = [
    ("empty", b"", 15, 18, 32),
    ("one_byte", b"a", 15, 18, 56),
    ("laozi_w12_b12", "laozi.txt", 12, 12, 10624),
    ("laozi_w15_b12", "laozi.txt", 15, 12, 10624),
    ("confucius_w15_b14", "confucius.txt", 15, 14, 29648),
    ("x64_w12_b16", "x64.elf", 12, 16, 478952),
    ("mandrill_w10_b18", "mandrill.bmp", 10, 18, 774840),
]
CASE_IDS = [c[0] for c in CASES]


def blocks_of(data: bytes, block_bits: int):
    bb = 1 << block_bits
    return [data[k:k + bb] for k in range(0, len(data), bb)]


def assemble(data: bytes, win_bits: int, block_bits: int, streams) -> bytes:
    blocks = blocks_of(data, block_bits)
    assert len(blocks) == len(streams) and all(len(s) % 8 == 0 for s in streams)
    index = b"".join(struct.pack("<II", len(s) // 8, zlib.crc32(b)) for s, b in zip(streams, blocks))
    head = struct.pack("<4sBBBBQQI", b"SQZF", 1, win_bits, block_bits, 0, len(data),
                       sum(len(s) for s in streams), len(blocks))
    front = head + struct.pack("<I", zlib.crc32(head + index)) + index
    return front + bytes(-len(front) % 16) + b"".join(streams)


def write_frame(data: bytes, win_bits: int, block_bits: int, encode=None) -> bytes:
    """encode(block) -> payload-only stream; the CPU oracle when not given"""
    if encode is None:
        encode = lambda blk: O.encode(blk, win_bits, header=False)
    return assemble(data, win_bits, block_bits, [encode(b) for b in blocks_of(data, block_bits)])


def case_data(name: str) -> bytes:
    src = next(c for c in CASES if c[0] == name)[1]
    return src if isinstance(src, bytes) else O.corpus(src)


@functools.lru_cache(maxsize=None)
def case_frame(name: str) -> bytes:
    """the writer's frame of a case (the oracle takes a few seconds for all of them: kept per process)"""
    _, _, wb, bits, _ = next(c for c in CASES if c[0] == name)
    return write_frame(case_data(name), wb, bits)


def fields(frame: bytes) -> dict:
    """the header as the writer laid it out (no checking)"""
    magic, ver, wb, bits, flags, content, payload, n, crc = struct.unpack("<4sBBBBQQII", frame[:32])
    off = (32 + 8 * n + 15) & ~15
    return {"content_bytes": content, "payload_bytes": payload, "payload_off": off, "frame_bytes": off + payload,
            "block_bytes": 1 << bits, "n_blocks": n, "win_bits": wb, "version": ver}


def reseal(frame: bytearray) -> bytes:
    """recompute index_crc over whatever header and index now say"""
    n = struct.unpack_from("<I", frame, 24)[0]
    struct.pack_into("<I", frame, 28, zlib.crc32(bytes(frame[:28]) + bytes(frame[32:32 + 8 * n])))
    return bytes(frame)


def refusals(frame: bytes):
    """(name, malformed frame, errno from the header alone, errno with the index in reach): each a valid frame of
    at least two blocks with ONE change"""
    f = fields(frame)
    assert f["n_blocks"] >= 2 and f["content_bytes"] % f["block_bytes"] > 1
    out = []

    def put(name, at, fmt, value, head_errno, full_errno):
        b = bytearray(frame)
        struct.pack_into(fmt, b, at, value)
        out.append((name, bytes(b), head_errno, full_errno))

    E = errno.EINVAL
    put("magic", 0, "<4s", b"SQZG", E, E)
    put("version_2", 4, "<B", 2, E, E)
    put("flags_1", 7, "<B", 1, E, E)
    put("win_bits_9", 5, "<B", 9, E, E)
    put("win_bits_16", 5, "<B", 16, E, E)
    put("block_bits_11", 6, "<B", 11, E, E)
    put("block_bits_25", 6, "<B", 25, E, E)
    put("n_blocks_plus_one", 24, "<I", f["n_blocks"] + 1, E, E)
    put("n_blocks_minus_one", 24, "<I", f["n_blocks"] - 1, E, E)
    # same number of blocks, so the header alone is consistent: only index_crc notices
    put("content_bytes_changed", 8, "<Q", f["content_bytes"] - 1, 0, errno.EILSEQ)
    b = bytearray(frame)
    b[32 + 8 + 5] ^= 0x10                                  # block 1's content_crc
    out.append(("index_bit_flipped", bytes(b), 0, errno.EILSEQ))
    b = bytearray(frame)
    words = struct.unpack_from("<I", b, 32)[0]
    struct.pack_into("<I", b, 32, words + 1)               # the sum no longer is payload_bytes / 8 ...
    out.append(("stream_words_sum", reseal(b), 0, E))      # ... under a checksum that is right
    return out
