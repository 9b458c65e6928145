"""CPU: the emit kernel's bit image (sqz_amd/csrc/huffman_emit.hip: BitQueue) now lives in LDS from one step to
the next and leaves in drains, not word by word after every step.  Nothing a caller sees may move: every stream,
`out_bytes` and `err` are held against the oracle on the CPU wave emulator (tests/emu/emu_emit_image.cpp), where
the output ends early too (the capacity, a malformed token), and not one byte is written at or behind a capacity
(guard bytes behind every slab).

The emulator build counts the drains of the image and the steps of the kernel's main loop; the long stream shows
that it was drained more than once, and fewer times than it took steps."""
import ctypes as C
import errno

import numpy as np
import pytest

import oracle_lib as O
import test_emu as TE

GUARD = 64
FILL = 0xA5
BAD_TOKEN = 0x1FF                  # no match bit and not a byte: neither the oracle nor token_ok takes it


def lib(variant="default"):
    return TE._build(variant, "emit_image")


def oracle(tokens, capacity=None):
    """stage 2 of the restatement on the token words -> (errno, its bytes)"""
    toks = np.ascontiguousarray(tokens, dtype=np.uint32)
    cap = 8 * len(toks) + 64 if capacity is None else capacity
    out = C.create_string_buffer(max(cap, 1))
    n, st = C.c_uint64(0), O.Stats()
    e = O.ORACLE.sqzo_encode_tokens(TE._p(toks), C.c_uint64(len(toks)), out, C.c_uint64(cap), C.byref(n), C.byref(st))
    return e, out.raw[:n.value]


def emit(E, tokens, capacity=None, prefix=(0, 0)):
    """one block through the emulated kernel -> (err, out_bytes, the slab's `capacity` bytes, drains, steps);
    the slab is aligned to 8 bytes and lies in front of GUARD bytes that must stay as they were"""
    toks = np.zeros(len(tokens) + 192, np.uint32)
    toks[:len(tokens)] = tokens
    cap = 8 * len(tokens) + 64 if capacity is None else capacity
    tok_off = np.array([0, max(len(tokens), 1)], np.uint64)
    cnt = np.array([len(tokens)], np.uint32)
    out_off = np.array([0, cap], np.uint64)
    raw = np.full(cap + GUARD + 8, FILL, np.uint8)
    shift = (-raw.ctypes.data) % 8
    out = raw[shift:shift + cap + GUARD]
    ob, err = np.zeros(1, np.uint64), np.full(1, -1, np.int32)
    drains, steps = C.c_uint32(0), C.c_uint32(0)
    E.emu_emit_image(TE._p(toks), TE._p(tok_off), TE._p(cnt), 1, C.c_void_p(out.ctypes.data), TE._p(out_off), TE._p(ob),
                     TE._p(err), C.c_uint64(prefix[0]), C.c_int(prefix[1]), C.byref(drains), C.byref(steps))
    assert (out[cap:] == FILL).all(), "bytes at or behind the capacity were written"
    assert (raw[:shift] == FILL).all()
    return int(err[0]), int(ob[0]), out[:cap].tobytes(), drains.value, steps.value


def same_as_oracle(E, tokens, capacity=None):
    e, want = oracle(tokens, capacity)
    err, nbytes, slab, drains, steps = emit(E, tokens, capacity)
    assert (err, nbytes) == (e, len(want)), (capacity, err, nbytes, e, len(want))
    assert slab[:nbytes] == want, capacity
    return e, want, drains, steps


@pytest.fixture(scope="module")
def laozi_tokens():
    return O.tokens(O.corpus("laozi.txt")[:6000], 1 << 12)


@pytest.fixture(scope="module")
def long_tokens():
    """a stream of several images: 2,400 tokens of Zipf bytes, about 18,000 bits"""
    return O.tokens(O.zipf_block(1, 8192), 1 << 12)[:2400]


def test_an_empty_block_and_a_one_token_block():
    E = lib()
    assert same_as_oracle(E, [])[:2] == (0, b"")
    e, want, _, _ = same_as_oracle(E, [65])
    assert e == 0 and len(want) == 8
    e, want, _, _ = same_as_oracle(E, [65, 66, 67, 0x80000000 | (9 << 16) | 3])     # ... and one with a back reference
    assert e == 0 and len(want) == 8


def last_one_bit(stream):
    """index of the last 1 bit of the stream (-1: none)"""
    v = int.from_bytes(stream, "big")
    return 8 * len(stream) - 1 - ((v & -v).bit_length() - 1) if v else -1


def test_streams_that_end_in_every_byte_of_a_word(laozi_tokens):
    """the payload's last 1 bit in byte 0..7 of the last word, and as the very last bit of it (the payload then
    ends exactly on the word boundary: nothing is left for the flush)"""
    E = lib()
    found = {}
    for n in range(120, 900):
        e, s = oracle(laozi_tokens[:n])
        assert e == 0
        last = last_one_bit(s)
        if last < 8 * len(s) - 64:                      # (a last word of zero bits does not say where the payload ends)
            continue
        key = "boundary" if last == 8 * len(s) - 1 else (last // 8) % 8
        found.setdefault(key, n)
        if len(found) == 9:
            break
    assert sorted(map(str, found)) == sorted(list("01234567") + ["boundary"]), found
    for key, n in found.items():
        e, _, _, _ = same_as_oracle(E, laozi_tokens[:n])
        assert e == 0, key


def bits_of(stream):
    return "".join(f"{b:08b}" for b in stream)


@pytest.mark.parametrize("fill", [1, 31, 63])
def test_header_bits_in_front_of_the_payload(laozi_tokens, fill):
    """the single-stream entry hands the kernel `fill` header bits that go in front: the stream is those bits, then
    the oracle's payload bits, in whole words.  The oracle's stream ends in up to 63 padding zeros, so the payload's
    length is known only between its last 1 bit and the end of its last word: the case takes a token count at which
    both give the same number of words."""
    E = lib()
    acc = 0x5A5A5A5A5A5A5A5B & ((1 << fill) - 1) | (1 << (fill - 1))
    for n in range(300, 400):
        e, s = oracle(laozi_tokens[:n])
        assert e == 0
        lo, hi = fill + last_one_bit(s) + 1, fill + 8 * len(s)
        if (lo + 63) // 64 == (hi + 63) // 64:
            break
    else:
        pytest.fail("no token count with a determined length")
    words = (lo + 63) // 64
    want_bits = (format(acc, f"0{fill}b") + bits_of(s)).ljust(64 * words + 64, "0")
    assert set(want_bits[64 * words:]) == {"0"}
    want = int(want_bits[:64 * words], 2).to_bytes(8 * words, "big")
    err, nbytes, slab, _, _ = emit(E, laozi_tokens[:n], prefix=(acc, fill))
    assert (err, nbytes) == (0, len(want))
    assert slab[:nbytes] == want


def test_a_long_stream_is_drained_more_than_once_and_not_every_step(long_tokens):
    E = lib()
    e, want, drains, steps = same_as_oracle(E, long_tokens)
    assert e == 0 and 8 * len(want) > 3 * 64 * 71      # more than three images of 71 words
    print("drains", drains, "steps", steps, "bytes", len(want))
    assert 3 < drains < steps, (drains, steps)         # (the end of the stream accounts for two drains at most)


def test_capacities_cut_the_stream_where_the_reference_stops(long_tokens):
    """the image holds 568 bytes: capacities below that end the stream before anything was drained, the others
    inside a later image; inside a word, on a word boundary, one word and one byte short of the whole stream, and
    the whole stream exactly"""
    E = lib()
    e, whole = oracle(long_tokens)
    assert e == 0 and len(whole) > 1500
    n = len(whole)
    seen = set()
    for cap in (0, 5, 8, 203, 208, 563, 568, 571, 1024, 1027, 1203, n - 9, n - 8, n - 1, n):
        e, want, _, _ = same_as_oracle(E, long_tokens, cap)
        assert e == (0 if cap == n else errno.E2BIG), cap
        assert len(want) == cap and want == whole[:cap]
        seen.add(e)
    assert seen == {0, errno.E2BIG}


@pytest.mark.parametrize("at", [0, 40, 1300])
def test_a_malformed_token_in_mid_stream(long_tokens, at):
    """EINVAL: the whole words in front of the token have left, the partial word has not"""
    E = lib()
    toks = np.concatenate([long_tokens[:at], np.array([BAD_TOKEN], np.uint32), long_tokens[at:at + 100]])
    e, want, _, _ = same_as_oracle(E, toks)
    assert e == errno.EINVAL and len(want) % 8 == 0
    if at == 1300:
        assert len(want) > 568                         # (behind the first drain)
        # ... and where the capacity ends such a stream first, it is the capacity's error
        e, _, _, _ = same_as_oracle(E, toks, 700)
        assert e == errno.E2BIG


def test_the_lowered_depth_build(long_tokens):
    """SQZ_AUX_DEPTH=7: the trees leave the batches early, codes and raw bits come from the one-at-a-time path
    through the pending register, whose fields are the widest a deposit takes (58 bits); the image is 64 words"""
    E = lib("shallow")
    e, want, drains, steps = same_as_oracle(E, long_tokens)
    assert e == 0 and 3 < drains < steps, (drains, steps)
    for cap in (203, 1027, len(want) - 8):
        e, _, _, _ = same_as_oracle(E, long_tokens, cap)
        assert e == errno.E2BIG
