"""GPU: SQZF version 2 (stored blocks) through the C ABI of libsqz_amd.so -- frames byte for byte against the
independent version-2 writer (tests/frame_writer_v2.py: struct + zlib + the CPU oracle, and the compiled reference
where oracle/_ref exists), host and device flavour, round trips over content that compresses in some blocks and not
in others, ranged reads across both kinds, refusals.

Corruption tests feed malformed DATA to hardened code: each shows that the refusal is an errno.
Nothing here reads the reference's tree: the GPU box does not have it."""
import ctypes as C
import errno
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import frame_writer as W
import frame_writer_v2 as W2
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BB = 1 << 18
S = W2.STORED


@pytest.fixture(scope="module")
def F():
    import torch
    assert torch.cuda.is_available()
    import sqz_amd
    assert "gfx950" in sqz_amd.device_info()["name"]
    from sqz_amd import frame
    return frame


@pytest.fixture(scope="module")
def L():
    from sqz_amd import _native
    return _native.lib()


def dev(t):
    import torch
    return torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda() if len(t) else torch.empty(0, dtype=torch.uint8, device="cuda")


def encode_on_device(F, data, wb, bits, store=True, capacity=None):
    enc = F.FrameEncoder(len(data), wb, bits, store=store, capacity=capacity)
    enc.encode(dev(data))
    return enc.result(), enc


def decode_on_device(F, frame, pattern=0x5A, info=None, trailing=0):
    """-> (bytes of d_out, err list, status); d_out is pre-filled with `pattern`"""
    import torch
    info = F.frame_info(frame[:32]) if info is None else info
    d_frame = dev(frame + bytes(trailing))
    d_out = torch.full((max(info["content_bytes"], 1),), pattern, dtype=torch.uint8, device="cuda")
    err, status = F.decode_frame(d_frame, d_out, info=info)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().tobytes()[:info["content_bytes"]], err.cpu().tolist(), int(status.item())


def stored_of(F, frame):
    return [b["stored"] for b in F.frame_blocks(frame)]


# ---------------------------------------------------------------- byte-exact frames
@pytest.mark.parametrize("name", W2.CASE_IDS)
def test_frames_equal_the_independent_writer(F, name):
    _, _, wb, bits = W2.case(name)[:4]
    data, want = W2.case_data(name), W2.case_frame(name)
    kinds = [b["stored"] for b in W2.blocks(want)]              # the writer's own choices, before the product's
    if name in W2.MIXED:
        assert 0 in kinds and 1 in kinds
    if name in W2.ALL_STORED:
        assert kinds and 0 not in kinds
    got = F.compress_frame(data, wb, bits, store=True)
    assert got == want
    on_device, _ = encode_on_device(F, data, wb, bits)
    assert on_device == got
    assert stored_of(F, got) == kinds
    assert F.decompress_frame(got) == data
    assert F.decompress_frame(got + b"trailing record") == data
    back, err, status = decode_on_device(F, got, trailing=40)
    assert status == 0 and not any(err) and back == data
    # flags = 0 through the _ex calls is the old call, byte for byte
    v1 = W2.case_frame_v1(name)
    assert F.compress_frame(data, wb, bits, store=False) == v1 == F.compress_frame(data, wb, bits)
    assert encode_on_device(F, data, wb, bits, store=False)[0] == v1
    assert F.decompress_frame(v1) == data


def test_flags_0_through_the_ex_calls_equals_the_old_calls(F, L):
    import torch
    data = W2.case_data("laozi_w15_b12")
    cap = L.sqz_frame_bound(len(data), 12)
    outs = []
    for call in ("old", "ex"):
        buf = (C.c_uint8 * cap)()
        n = C.c_uint64(0)
        if call == "old":
            assert L.sqz_frame_compress(data, len(data), 15, 12, buf, cap, C.byref(n)) == 0
        else:
            assert L.sqz_frame_compress_ex(data, len(data), 15, 12, 0, buf, cap, C.byref(n)) == 0
        outs.append(bytes(buf[:n.value]))
    assert outs[0] == outs[1] == W.case_frame("laozi_w15_b12")
    d_in = dev(data)
    need = L.sqz_hip_frame_scratch_bytes(len(data), 12, 1)
    assert need == L.sqz_hip_frame_scratch_bytes_ex(len(data), 12, 1, 0)
    frames = []
    for call in ("old", "ex"):
        d_frame = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        fb = torch.zeros(1, dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        err = torch.zeros(8, dtype=torch.int32, device="cuda")
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if call == "old":
            rc = L.sqz_hip_frame_encode(p(d_in), len(data), 15, 12, p(d_frame), cap, p(fb), p(st), p(err), p(scratch), need, stream)
        else:
            rc = L.sqz_hip_frame_encode_ex(p(d_in), len(data), 15, 12, 0, p(d_frame), cap, p(fb), p(st), p(err), p(scratch), need, stream)
        torch.cuda.synchronize()
        assert rc == 0 and int(st.item()) == 0
        frames.append(d_frame[:int(fb.item())].cpu().numpy().tobytes())
    assert frames[0] == frames[1] == outs[0]


@pytest.mark.skipif(O.REF is None, reason="oracle/_ref (the compiled reference) is not built here")
@pytest.mark.parametrize("name", ["mandrill_bmp_w10_b18", "laozi_w15_b12"])
def test_frames_equal_the_writer_over_the_compiled_reference(F, name):
    _, _, wb, bits = W2.case(name)[:4]
    data = W2.case_data(name)
    want = W2.write_frame(data, wb, bits, encode=lambda blk: O.ref_compress(blk, wb, header=False))
    assert want == W2.case_frame(name)
    assert F.compress_frame(data, wb, bits, store=True) == want


# ---------------------------------------------------------------- round trips
def _patchwork(nbytes, bits, seed, last_random):
    """whole blocks of noise, of Zipf bytes and of text in turn; the last (ragged) block as asked"""
    rng = random.Random(seed)
    bb = 1 << bits
    text = O.corpus("confucius.txt")
    noise = W2.random_bytes(nbytes + bb, seed)
    out, kinds = bytearray(), []
    while len(out) < nbytes:
        left = min(bb, nbytes - len(out))
        last = len(out) + left >= nbytes
        k = (1 if last_random else 2) if last else rng.randrange(3)
        if k == 1:
            out += noise[len(out):len(out) + left]
        elif k == 0:
            piece = bytearray()
            while len(piece) < left:
                piece += O.zipf_block(rng.randrange(1000), min(4000, left - len(piece)))
            out += piece[:left]
        else:
            a = rng.randrange(len(text) - 1)
            out += (text[a:] + text * (left // len(text) + 1))[:left]
        kinds.append(k)
    return bytes(out), kinds


@pytest.mark.parametrize("last_random", [False, True])
@pytest.mark.parametrize("bits,nbytes", [(12, 4096), (12, 4097), (12, 50001), (16, 65536), (16, 65537), (16, 300007),
                                         (18, (1 << 18) + 1), (20, (3 << 20) + 12345)])
def test_round_trips(F, bits, nbytes, last_random):
    data, kinds = _patchwork(nbytes, bits, bits * 1000 + nbytes % 997, last_random)
    frame = F.compress_frame(data, 13, bits, store=True)
    fi = F.frame_info(frame)
    assert fi["n_blocks"] == -(-nbytes // (1 << bits)) and fi["version"] == 2
    # Noise cannot be compressed, so a block of it is stored; a block of 4 KB or more of English text is not (laozi.txt
    # in 4 KB blocks stores none).  Zipf blocks and a short last block are left to the rule -- which the independent
    # writer applies to the oracle's streams where the content is small enough for the CPU.
    for k, blk in zip(kinds, F.frame_blocks(frame)):
        if k == 1 and blk["content_bytes"] >= 512:
            assert blk["stored"] == 1, blk
        if k == 2 and blk["content_bytes"] >= 4096:
            assert blk["stored"] == 0, blk
    if nbytes <= 300007:
        assert frame == W2.write_frame(data, 13, bits)
    assert len(frame) <= F.frame_bound(nbytes, bits, store=True)
    assert F.decompress_frame(frame) == data
    on_device, _ = encode_on_device(F, data, 13, bits)
    assert on_device == frame
    back, err, status = decode_on_device(F, frame)
    assert status == 0 and not any(err) and back == data


@pytest.fixture(scope="module")
def mixed(F):
    """16 blocks of 256 KB, every fourth one noise, the rest the bench generator's Zipf blocks, plus a ragged tail"""
    from sqz_amd import batch
    import torch
    z = batch.zipf_blocks(16, BB).cpu().numpy()
    torch.cuda.synchronize()
    noise = np.frombuffer(W2.random_bytes(4 * BB, 31), np.uint8)
    for k in range(4):
        z[(4 * k + 1) * BB:(4 * k + 2) * BB] = noise[k * BB:(k + 1) * BB]
    data = z.tobytes() + O.corpus("laozi.txt")[:5000]
    frame = F.compress_frame(data, 15, 18, store=True)
    want = [1 if b % 4 == 1 else 0 for b in range(16)] + [0]
    assert stored_of(F, frame) == want
    return data, frame, want


def test_read_range_across_both_kinds(F, mixed):
    data, frame, want = mixed
    n = len(data)
    pairs = [(BB - 10, 20), (BB + 100, 1000), (BB, BB), (2 * BB - 7, 14), (0, n), (n - 1, 1), (5 * BB - 3, 2 * BB + 9),
             (BB + 5, 0), (16 * BB - 1, 5001), (4 * BB + 17, 9 * BB)]
    rng = random.Random(77)
    for _ in range(40):
        a = rng.randrange(n)
        pairs.append((a, rng.randrange(min(n - a, 3 * BB) + 1)))
    for off, length in pairs:
        assert F.read_range(frame, off, length) == data[off:off + length], (off, length)
    # one stored block alone: no entropy decode work at all, the copy kernel's launch shows in the timing
    from sqz_amd import batch
    batch.set_timing(True)
    try:
        batch.get_timing(reset=True)
        assert F.read_range(frame, BB + 100, 1000) == data[BB + 100:BB + 1100]
        one = batch.get_timing(reset=True)
    finally:
        batch.set_timing(False)
    assert one["range_copy_kernel"][1] == 1 and one["entropy_decode_kernel"][1] == 1
    with pytest.raises(F.SqzError) as ei:
        F.read_range(frame, n, 1)
    assert ei.value.errno == errno.EINVAL


def test_two_host_passes_give_the_same_frame(F, mixed, monkeypatch):
    data, frame, _ = mixed
    monkeypatch.setenv("SQZ_FRAME_PASS_BYTES", str(3 * BB))        # 17 blocks in 6 passes, the last one short
    assert F.compress_frame(data, 15, 18, store=True) == frame
    assert F.decompress_frame(frame) == data
    assert F.read_range(frame, BB - 5, 4 * BB) == data[BB - 5:5 * BB - 5]


# ---------------------------------------------------------------- refusals
def _decompress_raw(L, frame, capacity=None, guard=64):
    fi = W.fields(frame)
    cap = fi["content_bytes"] if capacity is None else capacity
    store = bytearray(b"\xC3" * (cap + guard))
    out = (C.c_uint8 * (cap + guard)).from_buffer(store)
    errs = (C.c_int32 * max(fi["n_blocks"], 1))()
    n = C.c_uint64(0)
    rc = L.sqz_frame_decompress(frame, len(frame), out, cap, C.byref(n), errs)
    del out
    raw = bytes(store)
    return rc, raw[:cap], raw[cap:], list(errs)[:fi["n_blocks"]], n.value


def test_a_flipped_bit_in_a_stored_block_fails_that_block_only(F, L, mixed):
    data, frame, want = mixed
    k = 5
    blk = F.frame_blocks(frame)[k]
    assert blk["stored"] == 1
    bad = bytearray(frame)
    bad[blk["payload_off"] + blk["content_bytes"] // 2] ^= 0x04
    bad = bytes(bad)
    rc, out, guard, errs, _ = _decompress_raw(L, bad)
    assert rc == errno.EILSEQ and errs == [errno.EILSEQ if b == k else 0 for b in range(17)]
    assert out[:k * BB] == data[:k * BB] and out[(k + 1) * BB:] == data[(k + 1) * BB:]
    assert guard == b"\xC3" * 64
    back, derr, status = decode_on_device(F, bad)
    assert status == 0 and derr == errs
    assert back[:k * BB] == data[:k * BB] and back[(k + 1) * BB:] == data[(k + 1) * BB:]
    assert F.read_range(bad, (k + 1) * BB, 2 * BB + 17) == data[(k + 1) * BB:(k + 3) * BB + 17]
    with pytest.raises(F.SqzError):
        F.read_range(bad, k * BB + 3, 2)


@pytest.mark.parametrize("name", ["mandrill_bmp_w10_b18", "x64_w15_b12"])
def test_index_corruptions_are_refused_by_both_flavours(F, L, name):
    frame = W2.case_frame(name)
    good = W2.fields(frame)
    both = [r for r in W.refusals(frame) if r[0] not in ("version_2", "flags_1")] + W2.refusals(frame)
    for what, bad, head_errno, full_errno in both:
        rc, out, guard, errs, _ = _decompress_raw(L, bad, capacity=good["content_bytes"])
        assert rc == full_errno, what
        assert out == b"\xC3" * len(out) and guard == b"\xC3" * 64, what       # refused before anything is delivered
        info = dict(good)
        if head_errno == 0:
            info.update(W2.fields(bad))
        back, derr, status = decode_on_device(F, bad, info=info)
        want = full_errno if head_errno == 0 else errno.EINVAL
        assert status == want and derr == [want] * good["n_blocks"], what
        assert back == b"\x5A" * len(back), what                                # d_out untouched


# ---------------------------------------------------------------- the bound
def test_noise_fits_the_version_2_bound(F, L):
    import torch
    for nbytes, bits in ((65536, 12), (65537, 12), (BB * 3 + 5, 18), (9, 12)):
        data = W2.random_bytes(nbytes)
        n_blocks = -(-nbytes // (1 << bits))
        cap = F.frame_bound(nbytes, bits, store=True)
        assert cap == W2.pad16(32 + 8 * n_blocks) + W2.pad8(nbytes)
        frame = F.compress_frame(data, 15, bits, store=True)
        assert len(frame) == cap and all(stored_of(F, frame))          # every block stored: the bound is met exactly
        if nbytes < 100000:
            assert frame == W2.write_frame(data, 15, bits)
        on_device, enc = encode_on_device(F, data, 15, bits)           # the device flavour in a buffer of the bound
        assert enc.capacity == cap and on_device == frame
        v1 = F.compress_frame(data, 15, bits)
        # the version-1 frame is larger than its content; a stream of a few bytes can EQUAL the stored form (9 bytes:
        # 16 either way, and the rule stores on equality), a block of noise is larger
        assert F.frame_info(v1)["payload_bytes"] > nbytes and len(v1) >= len(frame)
        if nbytes >= 4096:
            assert len(v1) > len(frame)
        assert F.decompress_frame(frame) == data == F.decompress_frame(v1)
        # one byte less: E2BIG, the size still reported, nothing written
        enc2 = F.FrameEncoder(nbytes, 15, bits, store=True, capacity=cap - 8)
        enc2.frame.fill_(0xC3)
        enc2.encode(dev(data))
        torch.cuda.synchronize()
        assert int(enc2.status.item()) == errno.E2BIG and int(enc2.frame_bytes.item()) == cap
        assert bool((enc2.frame == 0xC3).all())
        buf = (C.c_uint8 * cap)()
        n = C.c_uint64(0)
        assert L.sqz_frame_compress_ex(data, nbytes, 15, bits, S, buf, cap - 8, C.byref(n)) == errno.E2BIG and n.value == cap


# ---------------------------------------------------------------- the decoder's wavefronts per stream
_WAVES_CHECK = r"""
import os, sys
sys.path.insert(0, os.environ["SQZ_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SQZ_ROOT"], "tests"))
import numpy as np, torch
import frame_writer_v2 as W2
from sqz_amd import frame as F
name = "mandrill_bmp_w15_b14"
data, frame = W2.case_data(name), W2.case_frame(name)
assert F.decompress_frame(frame) == data
assert F.read_range(frame, 16000, 40000) == data[16000:56000]
d_out = torch.full((len(data),), 0x5A, dtype=torch.uint8, device="cuda")
err, status = F.decode_frame(torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).cuda(), d_out)
torch.cuda.synchronize()
assert int(status.item()) == 0 and not err.cpu().numpy().any() and d_out.cpu().numpy().tobytes() == data
print("waves ok", os.environ.get("SQZ_DECODE_WAVES"))
"""


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_decoder_with_1_2_4_8_waves_on_a_mixed_frame(F, waves):
    """SQZ_DECODE_WAVES is read once per process: every setting in a fresh child process"""
    env = dict(os.environ, SQZ_DECODE_WAVES=str(waves), SQZ_ROOT=ROOT)
    p = subprocess.run([sys.executable, "-c", _WAVES_CHECK], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and f"waves ok {waves}" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# ---------------------------------------------------------------- full size
def test_full_size_mixed_frame(F):
    """1024 blocks of 256 KB, every fourth one noise, the rest the bench generator's Zipf blocks"""
    from sqz_amd import batch
    import torch
    n = 1024
    d = batch.zipf_blocks(n, BB)
    noise = torch.from_numpy(np.random.default_rng(41).integers(0, 256, (n // 4, BB), dtype=np.uint8)).cuda()
    d.view(n, BB)[3::4] = noise
    torch.cuda.synchronize()
    data = d.cpu().numpy()
    enc = F.FrameEncoder(n * BB, 15, 18, store=True)
    enc.encode(d)
    frame = enc.result()
    blocks = F.frame_blocks(frame)
    assert [b["stored"] for b in blocks] == [1 if b % 4 == 3 else 0 for b in range(n)]
    enc1 = F.FrameEncoder(n * BB, 15, 18)
    enc1.encode(d)
    v1 = enc1.result()
    sizes1 = [b["payload_bytes"] for b in F.frame_blocks(v1)]
    saved = sum(s - BB for s, b in zip(sizes1, blocks) if b["stored"])
    assert saved > 0 and all(s >= BB for s, b in zip(sizes1, blocks) if b["stored"])
    fi, fi1 = F.frame_info(frame), F.frame_info(v1)
    assert fi["payload_bytes"] == fi1["payload_bytes"] - saved
    assert [b["payload_bytes"] for b in blocks] == [BB if b["stored"] else s for s, b in zip(sizes1, blocks)]
    d_out = torch.full((n * BB,), 0x5A, dtype=torch.uint8, device="cuda")
    err, status = F.decode_frame(enc.frame[:len(frame)], d_out, info=fi)
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and not bool(err.any()) and torch.equal(d_out, d)
    d_out.fill_(0x5A)                                         # and the version-1 frame of the same content
    err, status = F.decode_frame(enc1.frame[:len(v1)], d_out, info=fi1)
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and not bool(err.any()) and torch.equal(d_out, d)
    assert F.read_range(frame, 3 * BB - 100, BB + 200) == data[3 * BB - 100:4 * BB + 100].tobytes()


# ---------------------------------------------------------------- the file tool
def test_file_tool_with_store(F, tmp_path):
    src = os.path.join(O.CORPUS, "mandrill.bmp")
    packed, back = str(tmp_path / "m.sqzf"), str(tmp_path / "m.back")
    run = lambda *a: subprocess.run([sys.executable, "-m", "sqz_amd.frame", *a], cwd=ROOT, capture_output=True,
                                    text=True, timeout=600)
    r = run("c", src, packed, "--win-bits", "10", "--block-bits", "18", "--store")
    assert r.returncode == 0, r.stdout + r.stderr
    want = W2.case_frame("mandrill_bmp_w10_b18")
    with open(packed, "rb") as fh:
        assert fh.read() == want
    r = run("d", packed, back)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(back, "rb") as fh:
        assert fh.read() == O.corpus("mandrill.bmp")
    r = run("blocks", packed)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4 and [int(l.split("stored=")[1]) for l in lines] == [b["stored"] for b in W2.blocks(want)]
    r = run("info", packed)
    assert r.returncode == 0, r.stdout + r.stderr
    said = {k: int(v) for k, v in (line.split(": ") for line in r.stdout.strip().splitlines())}
    assert said == W2.fields(want)
