"""TEST INFRASTRUCTURE: the shared inputs of the device-resident version-3 tests (test_frame_v3_emu.py,
test_frame_v3_gpu.py), written by the independent writer tests/frame_writer_v3.py over tests/dict_model.py.
Nothing here calls the product.  The model's match tables are computed once per (dictionary, block, window) and
shared by both parses and both store settings."""
import functools

import dict_model as DM
import frame_writer as W
import frame_writer_v2 as W2
import frame_writer_v3 as W3
import oracle_lib as O

RANGES = ((4090, 12), (8000, 400), (8500, 596))            # of the n = 3 content: across blocks 0|1, 1|2, inside block 2


@functools.lru_cache(maxsize=None)
def lao() -> bytes:
    return O.corpus("laozi.txt")


def dct() -> bytes:
    return lao()[:3000]


def mixed() -> bytes:
    """4 KB blocks: text, noise, a ragged block of text (the `framed` fixture of test_dict_gpu.py)"""
    return lao()[3000:7096] + W2.random_bytes(4096, 11) + lao()[7096:8000]


@functools.lru_cache(maxsize=None)
def _streams(dictionary: bytes, data: bytes, win_bits: int, block_bits: int):
    """{lazy: [stream per block]}"""
    out = {False: [], True: []}
    for b in W.blocks_of(data, block_bits):
        tab = DM.table(dictionary, b, 1 << win_bits)
        for lazy in (False, True):
            out[lazy].append(DM.LM.stream(DM.tokens(dictionary, b, 1 << win_bits, lazy, tab)))
    return out


def frame(dictionary: bytes, data: bytes, win_bits: int, block_bits: int, store: bool, lazy: bool) -> bytes:
    return W3.assemble(data, win_bits, block_bits, dictionary, _streams(dictionary, data, win_bits, block_bits)[lazy], store)


def streams(dictionary: bytes, data: bytes, win_bits: int, block_bits: int, lazy: bool):
    return _streams(dictionary, data, win_bits, block_bits)[lazy]


@functools.lru_cache(maxsize=None)
def contents():
    """[(name, win_bits, block_bits, dictionary, content)]"""
    text = lao()
    out = [("empty", 15, 12, dct(), b""),
           ("one_byte", 15, 12, dct(), b"x"),
           ("one_block", 15, 12, dct(), text[3000:7096]),
           ("two_blocks", 15, 12, dct(), text[3000:11192]),
           ("mixed", 15, 12, dct(), mixed()),
           ("w10", 10, 12, dct()[:1023], mixed()[:4097])]
    for name, window, dictionary, blocks, want in DM.cases(text, O.corpus("confucius.txt")):
        for k, b in enumerate(blocks):
            out.append((f"{name}_{k}", window.bit_length() - 1, 13, dictionary, b))
    return out


def check_layout():
    """what the shared inputs are there for, asserted from the writer before anything is compared"""
    by_name = {c[0]: c for c in contents()}

    def fr(name, store=False):
        _, wb, bb, d, data = by_name[name]
        return frame(d, data, wb, bb, store, False)

    f = W3.fields(fr("empty"))
    assert (f["n_blocks"], f["payload_off"], len(fr("empty"))) == (0, 48, 48)
    assert W3.fields(fr("one_byte"))["n_blocks"] == 1 and W3.blocks(fr("one_byte", True))[0]["stored"] == 1
    f = W3.fields(fr("one_block"))
    assert (f["n_blocks"], f["payload_off"]) == (1, 48)
    f = W3.fields(fr("two_blocks"))
    assert (f["n_blocks"], f["payload_off"]) == (2, 64) and fr("two_blocks")[56:64] == bytes(8)   # padding on even n
    assert [b["stored"] for b in W3.blocks(fr("mixed", True))] == [0, 1, 0]
    assert [b["stored"] for b in W3.blocks(fr("mixed", False))] == [0, 0, 0]
    assert {len(c[3]) for c in contents()} >= {1, 2, 3, 1023, 3000, 32767}
