"""GPU: the inputs of tests/test_bump_fold_emu.py (a literal node in the row the two trees share, offers cut at
a leaf without slack in every position the cut has a case for) through the device kernels: the token-level
entry sqz_hip_huffman_blocks, eight blocks per launch and one ragged launch of 70 blocks (more than the 16
streams a CU holds at once), the whole encoder on the byte block, and the decoders back.  Streams equal the
oracle's; the round trip is exact; the reference's tree fixtures at batch 64 through the tree entry."""
import os

import numpy as np
import pytest

import oracle_lib as O
import test_bump_fold_emu as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    import sqz_amd
    assert "gfx950" in sqz_amd.device_info()["name"]
    from sqz_amd import batch
    return torch, sqz_amd, batch


@pytest.fixture(scope="module")
def cases():
    """(name, tokens, the oracle's stream, the bytes the tokens stand for), computed once"""
    data = B.shared_row_block()
    out = [("shared_row_block", O.tokens(data, 1 << 12), O.encode(data, 12, header=False), data)]
    for name, (toks, _) in B.TOKEN_CASES.items():
        e, want, _ = O.encode_tokens(toks)
        assert e == 0
        out.append((name, np.asarray(toks, np.uint32), want, B.expand(toks)))
    return out


def emit_tokens(dev, blocks):
    torch, sq, batch = dev
    from sqz_amd import _native as N
    n = len(blocks)
    slots = max(len(b[3]) for b in blocks)                 # a block may not hold more tokens than bytes
    off = batch.uniform_offsets(n, slots)
    toks = np.zeros(n * slots + 64, np.uint32)
    counts = np.zeros(n, np.uint32)
    for k, (_, t, _, _) in enumerate(blocks):
        toks[k * slots:k * slots + len(t)] = t
        counts[k] = len(t)
    d_tok = torch.tensor(toks.view(np.int32), device="cuda")
    d_cnt = torch.tensor(counts.view(np.int32), device="cuda")
    cap = sq.bound(slots)
    out_off = batch.uniform_offsets(n, cap)
    out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    out_bytes = torch.zeros(n, dtype=torch.int64, device="cuda")
    err = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc = N.lib().sqz_hip_huffman_blocks(d_tok.data_ptr(), off.data_ptr(), d_cnt.data_ptr(), n, out.data_ptr(),
                                        out_off.data_ptr(), out_bytes.data_ptr(), err.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert err.cpu().numpy().tolist() == [0] * n
    h, nb = out.cpu().numpy(), out_bytes.cpu().numpy()
    return [h[k * cap:k * cap + int(nb[k])].tobytes() for k in range(n)]


@pytest.mark.parametrize("n_blocks", [8, 70])
def test_streams_equal_the_oracle_and_come_back(dev, cases, n_blocks):
    blocks = [cases[k % len(cases)] for k in range(n_blocks)]
    if n_blocks == 70:                                     # ragged: every third block stops short
        blocks = [(nm, t[:len(t) - 37 * (k % 3)], None, None) if k % 3 else (nm, t, w, d)
                  for k, (nm, t, w, d) in enumerate(blocks)]
        short = {}
        for k, (nm, t, w, d) in enumerate(blocks):
            if w is None:
                key = (nm, len(t))
                if key not in short:
                    e, want, _ = O.encode_tokens(t)
                    assert e == 0
                    short[key] = (want, B.expand(t))
                blocks[k] = (nm, t) + short[key]
    got = emit_tokens(dev, blocks)
    for k, (nm, _, want, _) in enumerate(blocks):
        assert got[k] == want, (k, nm)
    back, derr = dev[2].decode_blocks_host([b[2] for b in blocks], [len(b[3]) for b in blocks])
    assert derr.tolist() == [0] * n_blocks
    for k, (nm, _, _, data) in enumerate(blocks):
        assert back[k] == data, (k, nm)


def test_the_byte_block_through_the_whole_encoder(dev, cases):
    _, _, want, data = cases[0]
    outs, err = dev[2].encode_blocks_host([data] * 8, 1 << 12)
    assert err.tolist() == [0] * 8
    assert outs == [want] * 8


def test_reference_tree_dumps_at_batch_64(dev):
    import test_gpu_tree as T
    from sqz_amd import _native as N
    tdev = (dev[0], N.lib())
    z = np.load(os.path.join(O.GOLD, "trees.npz"))
    for name in sorted({k.split(".")[0] for k in z.files}):
        n = int(z[name + ".n"])
        syms = z[name + ".symbols"]
        ref = [z[f"{name}.{k}"] for k in ("freq", "path", "bits", "pix", "lix", "rix")]
        info = z[name + ".info"]
        if n == 8:
            ref, info = O.tree_run(O.ORACLE, "sqzo_tree_run", 32, syms)
            n = 32
        which, head, nodes = T.device_tree(tdev, n, syms, 64)
        T.compare(which, head, nodes, n, ref, info)
