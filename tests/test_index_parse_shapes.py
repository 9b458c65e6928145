"""index_parse_kernel, the shapes its tile loop can get wrong (lz77_index.hip): the indexed finder must give
the brute-force scan's tokens and the oracle's, token for token, in ONE launch over blocks that end just
before, at and just after a parse tile's edge -- including the lengths that put the block's last two positions
(literals taken from the bytes: they have no match word) on either side of the edge -- and over a block of
zeros, whose 257-byte tokens reach across chunk and tile boundaries all the way.  The parse walks tiles of
2048 positions (kTile), one position per byte; a tile's match words are fetched while the tile before is
walked, and its token words leave through LDS in a fixed number of stores, so the blocks around an edge are
where a clamped address or a carried entry point would show.  Window 2^10 keeps the oracle in seconds."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

WINDOW = 1 << 10
TILE = 2048          # positions per parse tile (kTile in sqz_amd/csrc/lz77_index.hip)


@pytest.fixture(scope="module")
def sq():
    import torch
    assert torch.cuda.is_available()
    import sqz_amd
    info = sqz_amd.device_info()
    assert "gfx950" in info["name"]
    return sqz_amd


def _check(sq, blocks):
    """one launch over `blocks`: index finder == scan finder == oracle, for every block"""
    import torch
    from sqz_amd import batch
    sizes = [len(b) for b in blocks]
    total = sum(sizes)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    d_in = torch.tensor(np.frombuffer(b"".join(blocks), np.uint8).copy(), device="cuda")
    off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    enc = batch.Encoder(len(blocks), total, sq.bound(max(sizes)))
    want = [O.tokens(b, WINDOW) for b in blocks]
    got = {}
    for finder in ("index", "scan"):
        toks, counts = enc.tokens(d_in, off, WINDOW, finder=finder)
        torch.cuda.synchronize()
        h_toks = toks.cpu().numpy().view(np.uint32)
        h_counts = counts.cpu().numpy()
        got[finder] = [h_toks[int(offs[k]):int(offs[k]) + int(h_counts[k])].copy() for k in range(len(blocks))]
    for k, w in enumerate(want):
        for finder in ("index", "scan"):
            g = got[finder][k]
            assert len(g) == len(w), (finder, k, sizes[k], len(g), len(w))
            assert (g == w).all(), (finder, k, sizes[k], int(np.argmax(g != w)))
        assert (got["index"][k] == got["scan"][k]).all(), (k, sizes[k])


def test_parse_tile_edges_and_long_tokens_in_one_launch(sq):
    edges = [k * TILE + d for k in (1, 2) for d in (-1, 0, 1, 2, 3)]
    blocks = [O.zipf_block(7 + n % 5, n) for n in edges]
    blocks.append(bytes(3 * TILE + 5))                       # zeros: 257-byte tokens across every tile boundary
    blocks.append(np.random.default_rng(5).integers(0, 256, 2 * TILE + 1, dtype=np.uint8).tobytes())   # all literals
    blocks.append((b"\x07\xf3\x80" * 3000)[:4 * TILE + 2])   # period three: long tokens that start off the chunk grid
    _check(sq, blocks)
