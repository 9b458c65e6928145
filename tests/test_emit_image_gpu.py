"""GPU: the emit kernel with its bit image kept in LDS from step to step (tests/test_emit_image_emu.py has the
cases on the emulator): eight blocks of 1 to 4 KB and one of 64 KB -- laozi.txt, Zipf bytes, uniform random bytes --
through the whole encoder, streams equal to the oracle's; and the token-level entry with capacities of about 1 KB
that end a stream inside a word, on a word boundary and before the image was ever drained: err, out_bytes and
the bytes below it are the oracle's, and nothing is written at or behind a capacity (every slab is followed by
the slab of an empty block, which must keep its fill)."""
import errno
import random

import numpy as np
import pytest

import oracle_lib as O
import test_emit_image_emu as EI

pytestmark = pytest.mark.gpu

WIN_BITS = 12
FILL = 0xA5


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    import sqz_amd
    assert "gfx950" in sqz_amd.device_info()["name"]
    from sqz_amd import batch
    return torch, sqz_amd, batch


@pytest.fixture(scope="module")
def blocks():
    laozi, rng = O.corpus("laozi.txt"), random.Random(11)
    small = [laozi[:1024], laozi[5000:5000 + 4096], laozi[12000:12000 + 2500],
             O.zipf_block(0, 1024), O.zipf_block(1, 4096), O.zipf_block(2, 3001),
             rng.randbytes(1024), rng.randbytes(4096)]
    big = laozi[:20480] + O.zipf_block(3, 24576) + rng.randbytes(20480)
    assert len(big) == 65536
    return small + [big]


def test_streams_equal_the_oracle(dev, blocks):
    outs, err = dev[2].encode_blocks_host(blocks, 1 << WIN_BITS)
    assert err.tolist() == [0] * len(blocks)
    for k, data in enumerate(blocks):
        assert outs[k] == O.encode(data, WIN_BITS, header=False), k


def test_capacities_at_one_kilobyte(dev, blocks):
    torch, sq, batch = dev
    from sqz_amd import _native as N
    toks = O.tokens(blocks[4], 1 << WIN_BITS)                   # 4 KB of Zipf bytes: a stream of about 3 KB
    e, whole = EI.oracle(toks)
    assert e == 0 and len(whole) > 2048
    caps = [200, 203, 563, 1024, 1027, 1029, len(whole) - 8, len(whole) - 1, len(whole)]
    # slab of case k, then the slab of an empty block (it brings the next slab back to a multiple of 8)
    n = 2 * len(caps)
    sizes = []
    for cap in caps:
        sizes += [cap, 64 + (-cap) % 8]
    out_off = np.zeros(n + 1, np.int64)
    out_off[1:] = np.cumsum(sizes)
    slots = len(toks) + 64
    tok = np.zeros(n * slots + 64, np.uint32)
    cnt = np.zeros(n, np.uint32)
    for k in range(len(caps)):
        tok[2 * k * slots:2 * k * slots + len(toks)] = toks
        cnt[2 * k] = len(toks)
    d_tok = torch.tensor(tok.view(np.int32), device="cuda")
    d_cnt = torch.tensor(cnt.view(np.int32), device="cuda")
    d_tok_off = batch.uniform_offsets(n, slots)
    d_out_off = torch.tensor(out_off, device="cuda")
    out = torch.full((int(out_off[-1]),), FILL, dtype=torch.uint8, device="cuda")
    out_bytes = torch.zeros(n, dtype=torch.int64, device="cuda")
    err = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc = N.lib().sqz_hip_huffman_blocks(d_tok.data_ptr(), d_tok_off.data_ptr(), d_cnt.data_ptr(), n, out.data_ptr(),
                                        d_out_off.data_ptr(), out_bytes.data_ptr(), err.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    h, nb, he = out.cpu().numpy(), out_bytes.cpu().numpy(), err.cpu().numpy()
    for k, cap in enumerate(caps):
        e, want = EI.oracle(toks, cap)
        assert e == (0 if cap == len(whole) else errno.E2BIG) and want == whole[:cap]
        at = int(out_off[2 * k])
        assert (int(he[2 * k]), int(nb[2 * k])) == (e, len(want)), cap
        assert h[at:at + len(want)].tobytes() == want, cap
        guard = h[int(out_off[2 * k + 1]):int(out_off[2 * k + 2])]
        assert (guard == FILL).all(), cap                      # nothing at or behind the capacity
        assert (int(he[2 * k + 1]), int(nb[2 * k + 1])) == (0, 0)
