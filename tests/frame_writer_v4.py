"""TEST INFRASTRUCTURE: an independent writer of SQZF VERSION-4 frames (include/sqz/sqz.h: the byte-shuffle filter) --
a numpy transposition per block, the CPU oracle (or tests/lazy_model.py) over the shuffled bytes, Python struct +
zlib.crc32 -- the closed-form inputs of the payload table, and the malformed version-4 variants the refusal tests
feed to the readers.  Nothing here calls the product.

Version 4 = version 2's layout, flags bit 2 (SHUFFLE), and one 8-byte record { elem_bytes, 0 } directly behind the
n index entries, covered by index_crc; payload_off = pad16(32 + 8n + 8).  Bit 0 (STORED) may accompany bit 2.  A
block's stream is the encoder's for S[j * m + i] = B[i * e + j], m = len(B) // e, the tail bytes behind the planes;
content_crc is over B; stored iff len(stream(S)) >= len(B), and a stored block carries B."""
import errno
import functools
import struct
import zlib

import numpy as np

import frame_writer as W
import lazy_model as LM
import oracle_lib as O

STORED = 1                 # flags bit 0
DICT = 2                   # flags bit 1
SHUFFLE = 4                # flags bit 2
STORED_BIT = 1 << 31       # of an index entry's first word
ELEMS = (2, 4, 8)
FIGURE_BYTES = 16389       # what every figure input is cut to: four blocks of 4 KB and five bytes (the i16 input,
                           # 6000 elements of 2 bytes, has 12000 and is not cut)


def pad16(n: int) -> int:
    return (n + 15) & ~15


def shuffle(block: bytes, e: int) -> bytes:
    m = len(block) // e
    a = np.frombuffer(block, np.uint8)
    return a[:m * e].reshape(m, e).T.tobytes() + block[m * e:]


def unshuffle(s: bytes, e: int) -> bytes:
    m = len(s) // e
    a = np.frombuffer(s, np.uint8)
    return a[:m * e].reshape(e, m).T.tobytes() + s[m * e:]


def stream_of(block: bytes, win_bits: int, lazy: bool = False) -> bytes:
    if not lazy:
        return O.encode(block, win_bits, header=False)
    return LM.stream(LM.parse(block, 1 << win_bits, True)[0])


def streams_of(data: bytes, win_bits: int, block_bits: int, e: int, lazy: bool = False, encode=None):
    if encode is None:
        encode = lambda s: stream_of(s, win_bits, lazy)
    return [encode(shuffle(b, e)) for b in W.blocks_of(data, block_bits)]


def assemble(data: bytes, win_bits: int, block_bits: int, e: int, streams, store: bool = False) -> bytes:
    blocks = W.blocks_of(data, block_bits)
    assert len(blocks) == len(streams) and all(len(s) % 8 == 0 for s in streams)
    index, payload = b"", []
    for s, b in zip(streams, blocks):
        stored = store and len(s) >= len(b)                 # the writer's rule of version 2, unchanged
        share = b + bytes(-len(b) % 8) if stored else s     # (a stored block is NOT shuffled)
        index += struct.pack("<II", len(share) // 8 | (STORED_BIT if stored else 0), zlib.crc32(b))
        payload.append(share)
    record = struct.pack("<II", e, 0)
    head = struct.pack("<4sBBBBQQI", b"SQZF", 4, win_bits, block_bits, SHUFFLE | (STORED if store else 0), len(data),
                       sum(len(p) for p in payload), len(blocks))
    front = head + struct.pack("<I", zlib.crc32(head + index + record)) + index + record
    return front + bytes(-len(front) % 16) + b"".join(payload)


@functools.lru_cache(maxsize=None)
def write_frame(data: bytes, win_bits: int, block_bits: int, e: int, store: bool = False, lazy: bool = False) -> bytes:
    return assemble(data, win_bits, block_bits, e, streams_of(data, win_bits, block_bits, e, lazy), store)


def fields(frame: bytes) -> dict:
    """the header and the record as laid out (no checking)"""
    magic, ver, wb, bits, flags, content, payload, n, crc = struct.unpack("<4sBBBBQQII", frame[:32])
    off = pad16(32 + 8 * n + 8)
    eb, zero = struct.unpack_from("<II", frame, 32 + 8 * n)
    return {"content_bytes": content, "payload_bytes": payload, "payload_off": off, "frame_bytes": off + payload,
            "block_bytes": 1 << bits, "n_blocks": n, "win_bits": wb, "version": ver, "flags": flags,
            "elem_bytes": eb, "zero": zero}


def blocks(frame: bytes) -> list:
    f = fields(frame)
    out, at = [], f["payload_off"]
    for b in range(f["n_blocks"]):
        word, crc = struct.unpack_from("<II", frame, 32 + 8 * b)
        share = 8 * (word & ~STORED_BIT)
        out.append({"payload_off": at, "payload_bytes": share,
                    "content_bytes": min(f["block_bytes"], f["content_bytes"] - b * f["block_bytes"]),
                    "content_crc": crc, "stored": word >> 31})
        at += share
    return out


def reseal(frame: bytearray) -> bytes:
    """recompute index_crc over whatever header, index and record now say"""
    n = struct.unpack_from("<I", frame, 24)[0]
    struct.pack_into("<I", frame, 28, zlib.crc32(bytes(frame[:28]) + bytes(frame[32:32 + 8 * n + 8])))
    return bytes(frame)


def refusals(frame: bytes):
    """(name, malformed frame, errno from the header alone, errno with index and record in reach): each a valid
    version-4 frame WITHOUT flags bit 0, of at least two blocks, with ONE change, resealed where index_crc must hold
    for the change to be reached"""
    f = fields(frame)
    assert f["version"] == 4 and f["flags"] == SHUFFLE and f["n_blocks"] >= 2
    n = f["n_blocks"]
    E = errno.EINVAL
    out = []

    def put(name, at, fmt, value, head_errno, full_errno, sealed=False):
        b = bytearray(frame)
        struct.pack_into(fmt, b, at, value)
        out.append((name, reseal(b) if sealed else bytes(b), head_errno, full_errno))

    put("v4_flags_0", 7, "<B", 0, E, E)                     # version 4 without bit 2
    put("v4_flags_1", 7, "<B", STORED, E, E)
    put("v4_flags_6", 7, "<B", SHUFFLE | DICT, E, E)        # bit 1 together with bit 2
    put("v4_flags_7", 7, "<B", SHUFFLE | DICT | STORED, E, E)
    for bit in range(3, 8):
        put(f"v4_flags_bit_{bit}", 7, "<B", SHUFFLE | (1 << bit), E, E)
    for v in (1, 2, 3):
        put(f"v{v}_flags_4", 4, "<B", v, E, E)              # versions 1..3 with bit 2
    put("version_5", 4, "<B", 5, E, E)
    for eb in (0, 1, 3, 5, 6, 16, 0x00010004):
        put(f"elem_bytes_{eb}", 32 + 8 * n, "<I", eb, 0, E, sealed=True)
    put("second_word_1", 32 + 8 * n + 4, "<I", 1, 0, E, sealed=True)
    put("record_stale_crc", 32 + 8 * n, "<I", 3, 0, errno.EILSEQ)     # a bad record under a stale checksum: EILSEQ first
    word = struct.unpack_from("<I", frame, 32)[0]
    put("stored_entry_without_bit_0", 32, "<I", word | STORED_BIT, 0, E, sealed=True)
    put("stream_words_sum", 32, "<I", word + 1, 0, E, sealed=True)
    put("payload_bytes_plus_8", 16, "<Q", f["payload_bytes"] + 8, 0, E, sealed=True)
    put("index_bit_flipped", 32 + 8 + 5, "<B", frame[32 + 8 + 5] ^ 0x10, 0, errno.EILSEQ)
    return out


# ---- the closed-form inputs of the payload table (i = 0..5999, little-endian, cut to FIGURE_BYTES)
def _i():
    return np.arange(6000, dtype=np.uint64)


def _cut(a) -> bytes:
    return a.tobytes()[:FIGURE_BYTES]


@functools.lru_cache(maxsize=None)
def figure_input(name: str) -> bytes:
    i = _i()
    if name == "u32_ramp":
        return _cut((7 * i + ((i * i >> np.uint64(7)) & np.uint64(63))).astype("<u4"))
    if name == "f32_sine":
        return _cut(np.sin(i.astype(np.float64) / 50).astype("<f4"))
    if name == "i16_sine_noise":
        s = np.round(8000 * np.sin(i.astype(np.float64) / 30)).astype(np.int64)
        return _cut((s + ((i * np.uint64(2654435761) >> np.uint64(7)) & np.uint64(31)).astype(np.int64)).astype("<i2"))
    if name == "u64_stamps":
        return _cut((np.uint64(1700000000000) + 997 * i + ((i * i >> np.uint64(9)) & np.uint64(127))).astype("<u8"))
    if name == "u32_noise":
        with np.errstate(over="ignore"):                    # 64-bit arithmetic, truncated
            return _cut(((i * np.uint64(2654435761) * (i + np.uint64(12345))) >> np.uint64(11)).astype("<u4"))
    raise KeyError(name)


# (name, element bytes); the filter helps the first four, the last is noise
FIGURES = [("u32_ramp", 4), ("f32_sine", 4), ("i16_sine_noise", 2), ("u64_stamps", 8), ("u32_noise", 4)]


@functools.lru_cache(maxsize=None)
def model_payload(name: str, e: int, block_bits: int, win_bits: int = 15) -> int:
    """payload bytes of the frame without stored blocks: e = 0 plain (version 1), else shuffled (version 4)"""
    data = figure_input(name)
    if e == 0:
        return sum(len(stream_of(b, win_bits)) for b in W.blocks_of(data, block_bits))
    return sum(len(s) for s in streams_of(data, win_bits, block_bits, e))
