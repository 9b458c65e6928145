"""TEST INFRASTRUCTURE: the batch with byte-shuffled (version 4) frames in it that tests/test_frames_v4_*.py share --
nine contents cut from tests/frame_writer_v4.py's closed-form inputs, one element size per frame, and the frames the
independent writers (tests/frame_writer.py, _v2.py, _v4.py) make of them over the CPU oracle.  Nothing here calls the
product."""
import functools

import frame_writer as W
import frame_writer_v2 as W2
import frame_writer_v4 as W4

WB, BITS = 15, 12
BB = 1 << BITS
ELEMS = [4, 0, 2, 8, 0, 4, 2, 4, 0]
K = len(ELEMS)
# 0, 1, e - 1 (of the frame it belongs to: e = 2), a block, a block and a byte, three blocks and five bytes, the whole
# figure input, a block less a byte, two blocks
LENGTHS = [0, 1, ELEMS[2] - 1, BB, BB + 1, 3 * BB + 5, W4.FIGURE_BYTES, BB - 1, 2 * BB]
# the e = 8 frame carries the f32 sine, which the block encoder takes shuffled by 8 (the u64 time stamps it does not:
# E2BIG from the emit kernel's tree guard); the hashed u32 is noise, which a version with stored blocks stores
INPUTS = ["u32_ramp", "u32_noise", "i16_sine_noise", "f32_sine", "u32_ramp", "u32_ramp", "i16_sine_noise", "u32_noise",
          "f32_sine"]


@functools.lru_cache(maxsize=None)
def content(f: int) -> bytes:
    data = W4.figure_input(INPUTS[f])
    data = data * (LENGTHS[f] // len(data) + 1)              # the i16 input is 12000 bytes: once more behind itself
    return data[:LENGTHS[f]]


def contents():
    return [content(f) for f in range(K)]


@functools.lru_cache(maxsize=None)
def written(data: bytes, e: int, store: bool, win_bits: int = WB, block_bits: int = BITS) -> bytes:
    """the independent writers' frame: version 4 where e != 0, else version 2 with store and version 1 without"""
    if e != 0:
        return W4.write_frame(data, win_bits, block_bits, e, store)
    if store:
        return W2.write_frame(data, win_bits, block_bits)
    return W.write_frame(data, win_bits, block_bits)


@functools.lru_cache(maxsize=None)
def streams(f: int):
    """what the block encoder makes of frame f's blocks: of the shuffled bytes where the frame is shuffled"""
    if ELEMS[f] != 0:
        return tuple(W4.streams_of(content(f), WB, BITS, ELEMS[f]))
    return tuple(W4.stream_of(b, WB) for b in W.blocks_of(content(f), BITS))


def frames(store: bool):
    return [written(content(f), ELEMS[f], store) for f in range(K)]


def pad8(n):
    return (n + 7) & ~7


def pad16(n):
    return (n + 15) & ~15


def blocks_in(c, bits=BITS):
    return (c + (1 << bits) - 1) >> bits


def sqz_bound(n):
    return (2 * n + 1024 + 7) & ~7


def frame_bound(c, bits, store, e=0):
    """sqz_frame_bound_ex, and sqz_frame_bound_shuf where e != 0: the record's 8 bytes in front of the padding"""
    bb = 1 << bits
    off = pad16(32 + 8 * blocks_in(c, bits) + (8 if e else 0))
    if store:
        return off + pad8(c)
    return off + (c // bb) * sqz_bound(bb) + (sqz_bound(c % bb) if c % bb else 0)


def layout(sizes, elems, bits, store):
    """(in_at, frame_at, base): k + 1 entries each"""
    in_at, frame_at, base = [0], [0], [0]
    for c, e in zip(sizes, elems):
        in_at.append(in_at[-1] + c)
        frame_at.append(frame_at[-1] + pad16(frame_bound(c, bits, store, e)))
        base.append(base[-1] + blocks_in(c, bits))
    return in_at, frame_at, base


def fields(frame: bytes) -> dict:
    """the header as laid out, with payload_off by the version (a record behind the index of versions 3 and 4)"""
    f = W.fields(frame)
    if f["version"] >= 3:
        f = dict(f, payload_off=pad16(32 + 8 * f["n_blocks"] + 8))
    return f


def blocks(frame: bytes) -> list:
    return W4.blocks(frame) if frame[4] == 4 else W2.blocks(frame)
