"""GPU: a shared dictionary through every layer, against tests/dict_model.py (the oracle's finder over Dct || B, its
tokens through the oracle's coder) and the independent version-3 writer (tests/frame_writer_v3.py).

The inputs are dict_model.cases(): a handful of blocks of at most 5,000 bytes in which the corners are planted --
a source in the dictionary's last two bytes, one that straddles its end, a periodic copy out of it, a dictionary
match as a block's first token, a match of 257, a tie the block keeps, window 2^10 with D = 1023, D = 32767 with
blocks of 4,096 and 5,000 bytes, D of 1, 2 and 3, blocks of 0..3 bytes and a short last block.  That they are on the
path is asserted from the model's tokens before anything is compared.  The model's results are computed once."""
import ctypes as C
import errno
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import dict_model as DM
import frame_writer as W
import frame_writer_v2 as W2
import frame_writer_v3 as W3
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOK_MATCH = DM.TOK_MATCH
PARSES = ((False, "greedy"), (True, "lazy"))


@pytest.fixture(scope="module")
def B():
    import torch
    assert torch.cuda.is_available()
    import sqz_amd
    assert "gfx950" in sqz_amd.device_info()["name"]
    from sqz_amd import batch
    return batch


@pytest.fixture(scope="module")
def F(B):
    from sqz_amd import frame
    return frame


@pytest.fixture(scope="module")
def L(B):
    from sqz_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def lao():
    return O.corpus("laozi.txt")


@pytest.fixture(scope="module")
def cases(lao):
    """(name, window, dictionary, blocks, {lazy: tokens per block}, {lazy: streams per block})"""
    out, seen = [], set()
    for name, window, dct, blocks, want in DM.cases(lao, O.corpus("confucius.txt")):
        tabs = [DM.table(dct, b, window) for b in blocks]
        toks = {lazy: [DM.tokens(dct, b, window, lazy, t) for b, t in zip(blocks, tabs)] for lazy in (False, True)}
        streams = {lazy: [DM.LM.stream(t) for t in toks[lazy]] for lazy in (False, True)}
        got = DM.corners(toks[False][0], len(dct))
        assert want <= got, (name, want - got)
        seen |= got
        if name == "long_and_tie":
            assert len(DM.ties_kept_in_block(dct, blocks[0], window, toks[False][0])) > 0
        if name == "w10":                                  # position 1 is the dictionary's position 0: one byte out of reach
            assert O.match_at(dct + blocks[0], len(dct) + 1, 2 * window) == (257, 1024) and tabs[0][0][1] < 257
        for lazy in (False, True):
            assert [DM.expand(t, dct) for t in toks[lazy]] == blocks
        out.append((name, window, dct, blocks, toks, streams))
    assert {"source_at_D-1", "source_at_D-2", "straddle", "periodic_from_dict", "first_token", "len_257"} <= seen
    assert any(len(b) < 4 for c in out for b in c[3]) and {len(c[2]) for c in out} >= {1, 2, 3, 1023, 32767}
    return out


def _dev(blocks):
    import torch
    sizes = [len(b) for b in blocks]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    data = np.frombuffer(b"".join(blocks) + bytes(64), np.uint8).copy()
    return torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda(), off, sizes


def _streams_of(out, out_off, out_bytes, n):
    nb, oo, raw = out_bytes.cpu().numpy(), out_off.cpu().numpy(), out.cpu().numpy()
    return [raw[int(oo[k]):int(oo[k]) + int(nb[k])].tobytes() for k in range(n)]


# ---------------------------------------------------------------- tokens and streams against the model
def test_tokens_equal_the_model(B, cases):
    import torch
    for name, window, dct, blocks, toks, streams in cases:
        d_in, d_off, off, sizes = _dev(blocks)
        enc = B.Encoder(len(blocks), int(off[-1]), 64)
        for lazy, parse in PARSES:
            got, counts = enc.tokens(d_in, d_off, window, parse=parse, dictionary=dct)
            torch.cuda.synchronize()
            got, counts = got.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)
            for k, want in enumerate(toks[lazy]):
                assert int(counts[k]) == len(want), (name, parse, k, int(counts[k]), len(want))
                mine = got[int(off[k]):int(off[k]) + len(want)]
                assert (mine == want).all(), (name, parse, k, int(np.argmax(mine != want)))


def test_streams_equal_the_model_and_decode_back(B, cases):
    import torch
    for name, window, dct, blocks, toks, streams in cases:
        d_in, d_off, off, sizes = _dev(blocks)
        cap = max(int(B.N.lib().sqz_bound(max(sizes + [1]))), 64)
        enc = B.Encoder(len(blocks), int(off[-1]), cap)
        for lazy, parse in PARSES:
            out, out_off, out_bytes, err = enc.encode(d_in, d_off, window, parse=parse, dictionary=dct)
            torch.cuda.synchronize()
            assert not err.cpu().numpy().any(), (name, parse)
            assert _streams_of(out, out_off, out_bytes, len(blocks)) == streams[lazy], (name, parse)
            back = torch.full((int(off[-1]) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            derr = B.decode_blocks(out, out_off, len(blocks), back, d_off, dictionary=dct)
            torch.cuda.synchronize()
            assert not derr.cpu().numpy().any(), (name, parse)
            back = back.cpu().numpy()
            assert back[:int(off[-1])].tobytes() == b"".join(blocks) and (back[int(off[-1]):] == 0x5A).all(), (name, parse)
            # the host flavour: the same streams, and the model's streams back to the content
            outs, herr = B.encode_blocks_host(blocks, window, parse=parse, dictionary=dct)
            assert not herr.any() and outs == streams[lazy], (name, parse)
            texts, herr = B.decode_blocks_host(streams[lazy], sizes, dictionary=dct)
            assert not herr.any() and texts == blocks, (name, parse)
        # the dictionary is what makes these streams: the plain decoder refuses them (dist > position) or gives other bytes
        texts, herr = B.decode_blocks_host(streams[False][:1], sizes[:1])
        assert herr[0] == errno.EINVAL or texts[0] != blocks[0], name


def test_the_calls_without_a_dictionary_still_give_the_oracles_streams(B, cases):
    for name, window, dct, blocks, toks, streams in cases:
        wb = window.bit_length() - 1
        want = [O.encode(b, wb, header=False) for b in blocks]
        outs, err = B.encode_blocks_host(blocks, window)
        assert not err.any() and outs == want, name
        texts, err = B.decode_blocks_host(want, [len(b) for b in blocks])
        assert not err.any() and texts == blocks, name
        if len(dct) >= 500:                                # (a dictionary of text never costs these blocks a word)
            assert sum(map(len, streams[False])) <= sum(map(len, want)), name


# ---------------------------------------------------------------- the decoder with 1, 2, 4 and 8 waves
_REFUSED = {
    # dictionary "0123456789": position 2 + D reaches "0123"; one byte further does not; nor does D + 1 at position 0
    "ok": [ord("a"), ord("b"), TOK_MATCH | (4 << 16) | 12, ord("c")],
    "bad": [ord("a"), ord("b"), TOK_MATCH | (4 << 16) | 13, ord("c")],
    "first": [TOK_MATCH | (3 << 16) | 11, ord("c")],
}

_WAVES_CHECK = r"""
import os, pickle, sys
sys.path.insert(0, os.environ["SQZ_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SQZ_ROOT"], "tests"))
import numpy as np, torch
from sqz_amd import batch, frame as F
with open(os.environ["SQZ_DICT_CASES"], "rb") as fh:
    jobs, refused, framed = pickle.load(fh)
for name, dct, blocks, streams in jobs:
    sizes = [len(b) for b in blocks]
    texts, err = batch.decode_blocks_host(streams, sizes, dictionary=dct)
    assert not err.any() and texts == blocks, (name, err.tolist())
    in_off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    comp = torch.from_numpy(np.frombuffer(b"".join(streams) + bytes(64), np.uint8).copy()).cuda()
    back = torch.full((int(out_off[-1]) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    derr = batch.decode_blocks(comp, torch.from_numpy(in_off).cuda(), len(blocks), back, torch.from_numpy(out_off).cuda(),
                               dictionary=dct)
    torch.cuda.synchronize()
    assert not derr.cpu().numpy().any() and back.cpu().numpy()[:int(out_off[-1])].tobytes() == b"".join(blocks), name
dct, streams, sizes = refused
texts, err = batch.decode_blocks_host(streams, sizes, dictionary=dct)
assert err.tolist() == [0, 22, 22, 0], err.tolist()
assert texts[0] == b"ab0123c" and texts[3] == b"plain literals, then nothing"
texts, err = batch.decode_blocks_host(streams, sizes)
assert err.tolist() == [22, 22, 22, 0], err.tolist()
dct, data, frame = framed
assert F.decompress_frame(frame, dictionary=dct) == data and F.read_range(frame, 4000, 300, dictionary=dct) == data[4000:4300]
print("waves ok", os.environ.get("SQZ_DECODE_WAVES"))
"""


@pytest.fixture(scope="module")
def waves_file(cases, lao, tmp_path_factory):
    lit = np.frombuffer(b"plain literals, then nothing", np.uint8).astype(np.uint32)
    refused = [DM.LM.stream(np.array(_REFUSED[k], np.uint32)) for k in ("ok", "bad", "first")] + [DM.LM.stream(lit)]
    jobs = [(name, dct, blocks, streams[lazy]) for name, window, dct, blocks, toks, streams in cases for lazy in (False, True)]
    dct, data = lao[:3000], lao[3000:7096] + W2.random_bytes(4096, 11) + lao[7096:8000]
    p = tmp_path_factory.mktemp("dict") / "cases.pickle"
    with open(p, "wb") as fh:
        pickle.dump((jobs, (b"0123456789", refused, [7, 7, 4, len(lit)]),
                     (dct, data, W3.write_frame(data, 15, 12, dct, store=True))), fh)
    return str(p)


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_decoder_with_1_2_4_8_waves_per_stream(B, waves_file, waves):
    """SQZ_DECODE_WAVES is read once per process: every setting in a fresh child process, which decodes the model's
    streams of every case (host and device flavour), the streams whose distance reaches in front of the dictionary
    (EINVAL, as dist > position is without one) and a version-3 frame with a stored block"""
    env = dict(os.environ, SQZ_DECODE_WAVES=str(waves), SQZ_ROOT=ROOT, SQZ_DICT_CASES=waves_file)
    p = subprocess.run([sys.executable, "-c", _WAVES_CHECK], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and f"waves ok {waves}" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# ---------------------------------------------------------------- frames
@pytest.fixture(scope="module")
def framed(lao):
    """dictionary, content (4 KB blocks: text, noise, a ragged block of text), and the writer's frames"""
    dct = lao[:3000]
    data = lao[3000:7096] + W2.random_bytes(4096, 11) + lao[7096:8000]
    want = {(store, lazy): W3.write_frame(data, 15, 12, dct, store=store, lazy=lazy)
            for store in (False, True) for lazy in (False, True)}
    assert [b["stored"] for b in W3.blocks(want[True, False])] == [0, 1, 0]
    return dct, data, want


def test_frames_equal_the_independent_writer(F, framed, monkeypatch):
    dct, data, want = framed
    for (store, lazy), frame in want.items():
        got = F.compress_frame(data, 15, 12, store=store, parse="lazy" if lazy else "greedy", dictionary=dct)
        assert got == frame, (store, lazy)
        assert F.frame_info(got) == W3.fields(frame) and F.frame_blocks(got) == W3.blocks(frame)
        assert F.decompress_frame(got, dictionary=dct) == data
        # across the edges of blocks 0 | 1 (a stored block when store) and 1 | 2, and a range inside the ragged block
        for at, n in ((4090, 12), (8000, 400), (8500, 596), (0, len(data)), (len(data), 0)):
            assert F.read_range(got, at, n, dictionary=dct) == data[at:at + n], (store, lazy, at)
    # one block per pass: the same frame, the same content (the dictionary is uploaded and indexed once per call)
    monkeypatch.setenv("SQZ_FRAME_PASS_BYTES", "4096")
    assert F.compress_frame(data, 15, 12, store=True, dictionary=dct) == want[True, False]
    assert F.decompress_frame(want[True, False], dictionary=dct) == data
    monkeypatch.delenv("SQZ_FRAME_PASS_BYTES")
    # window 2^10 with the largest dictionary it admits, a single ragged block, a block of one byte
    d10 = dct[:1023]
    for content in (data[:300], b"x", data[:4097]):
        for store in (False, True):
            got = F.compress_frame(content, 10, 12, store=store, dictionary=d10)
            assert got == W3.write_frame(content, 10, 12, d10, store=store), (len(content), store)
            assert F.decompress_frame(got, dictionary=d10) == content


def test_a_frame_without_a_dictionary_is_what_it_was(F, lao):
    with open(os.path.join(O.GOLD, "laozi.txt.w15.b12.sqzf"), "rb") as fh:
        golden = fh.read()
    assert F.compress_frame(lao, 15, 12) == golden == W.write_frame(lao, 15, 12)
    assert F.decompress_frame(golden) == lao and F.frame_info(golden)["dict_bytes"] == 0


def test_readers_refuse_the_wrong_dictionary_and_the_wrong_call(F, L, framed):
    dct, data, want = framed
    frame = want[True, False]
    wrong = bytes([dct[0] ^ 1]) + dct[1:]                  # the right length, one bit off
    out = (C.c_uint8 * len(data))(*([0x5A] * len(data)))
    errs = (C.c_int32 * 3)(-1, -1, -1)
    n = C.c_uint64(0)
    for bad in (wrong, dct[:-1], dct + b"x"):
        rc = L.sqz_frame_decompress_dict(frame, len(frame), bad, len(bad), out, len(data), C.byref(n), errs)
        assert rc == errno.EILSEQ and list(errs) == [errno.EILSEQ] * 3
        assert L.sqz_frame_read_dict(frame, len(frame), bad, len(bad), 100, 200, out) == errno.EILSEQ
        assert bytes(out) == b"\x5a" * len(data)           # nothing decoded, nothing written
        with pytest.raises(OSError) as e:
            F.decompress_frame(frame, dictionary=bad)
        assert e.value.errno == errno.EILSEQ and e.value.block_errors == [errno.EILSEQ] * 3
    # the old readers on a version-3 frame, the new ones on the others
    assert L.sqz_frame_decompress(frame, len(frame), out, len(data), C.byref(n), errs) == errno.EINVAL
    assert L.sqz_frame_read(frame, len(frame), 100, 200, out) == errno.EINVAL
    assert bytes(out) == b"\x5a" * len(data)
    for plain in (W.write_frame(data, 15, 12), W2.write_frame(data, 15, 12)):
        assert L.sqz_frame_decompress_dict(plain, len(plain), dct, len(dct), out, len(data), C.byref(n), errs) == errno.EINVAL
        assert L.sqz_frame_read_dict(plain, len(plain), dct, len(dct), 100, 200, out) == errno.EINVAL
    assert bytes(out) == b"\x5a" * len(data)
    # a damaged block: its errno for that block, the others delivered
    bad = bytearray(frame)
    bad[W3.blocks(frame)[2]["payload_off"] + 9] ^= 0x40
    text, block_errors = F.decompress_frame(bytes(bad), return_errors=True, dictionary=dct)
    assert block_errors[:2] == [0, 0] and block_errors[2] != 0 and text[:8192] == data[:8192]


def test_the_device_frame_calls_do_not_know_version_3(F, L, framed):
    import torch
    dct, data, want = framed
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    for store in (False, True):
        enc = F.FrameEncoder(len(data), 15, 12, store=store)
        for flags in (W3.DICT, W3.DICT | W3.STORED):
            rc = L.sqz_hip_frame_encode_ex(d_in.data_ptr(), len(data), 15, 12, flags, enc.frame.data_ptr(), enc.capacity,
                                           enc.frame_bytes.data_ptr(), enc.status.data_ptr(), enc.err.data_ptr(),
                                           enc.scratch.data_ptr(), enc.scratch_bytes, None)
            assert rc == errno.EINVAL
    # the decode refuses a version-3 frame by arithmetic: a status, every block's errno, nothing written
    frame = want[True, False]
    d_frame = torch.from_numpy(np.frombuffer(frame + bytes(64), np.uint8).copy()).cuda()
    d_out = torch.full((len(data),), 0x5A, dtype=torch.uint8, device="cuda")
    err, status = F.decode_frame(d_frame, d_out, info=W3.fields(frame))
    torch.cuda.synchronize()
    assert int(status.item()) == errno.EINVAL and err.cpu().numpy().tolist() == [errno.EINVAL] * 3
    assert (d_out.cpu().numpy() == 0x5A).all()


def test_file_tool_round_trip(F, framed, tmp_path, capsys):
    dct, data, want = framed
    (tmp_path / "in").write_bytes(data)
    (tmp_path / "dict").write_bytes(dct)
    src, dfile, packed, back = (str(tmp_path / k) for k in ("in", "dict", "packed", "back"))
    assert F.main(["c", src, packed, "--block-bits", "12", "--store", "--dict", dfile]) == 0
    with open(packed, "rb") as fh:
        assert fh.read() == want[True, False]
    capsys.readouterr()
    assert F.main(["info", packed]) == 0
    out = capsys.readouterr().out
    assert "version: 3" in out and f"dict_bytes: {len(dct)}" in out and f"dict_crc: {W3.fields(want[True, False])['dict_crc']}" in out
    assert F.main(["d", packed, back, "--dict", dfile]) == 0
    with open(back, "rb") as fh:
        assert fh.read() == data
    assert F.main(["d", packed, back]) == 1                 # no dictionary: refused, with a message
    (tmp_path / "other").write_bytes(dct[::-1])
    assert F.main(["d", packed, back, "--dict", str(tmp_path / "other")]) == 1
