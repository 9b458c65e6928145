"""index_sort_kernel, the shapes its tile loop can get wrong (lz77_index.hip): the indexed finder must give
the brute-force scan's tokens and the oracle's, token for token, for blocks that end just before, at and just
after a tile boundary, for a tile whose elements all carry one digit, for digits that are all about equally
full, and for one launch whose blocks differ in length.  Every pass of the kernel orders tiles of 4096
positions (kSortTile; pass 0 has no tile size of its own), and a block of n bytes has n - 2 positions: its
two last bytes have no 3-byte key.  Window 2^10 keeps the oracle in seconds."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

WINDOW = 1 << 10
TILE = 4096          # positions per tile of every pass (kSortTile in sqz_amd/csrc/lz77_index.hip)


@pytest.fixture(scope="module")
def sq():
    import torch
    assert torch.cuda.is_available()
    import sqz_amd
    info = sqz_amd.device_info()
    assert "gfx950" in info["name"]
    return sqz_amd


@pytest.fixture(scope="module")
def batch(sq):
    from sqz_amd import batch as b
    return b


def _random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _check(sq, batch, blocks):
    """one launch over `blocks`: index finder == scan finder == oracle, for every block"""
    import torch
    sizes = [len(b) for b in blocks]
    total = sum(sizes)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    d_in = torch.tensor(np.frombuffer(b"".join(blocks), np.uint8).copy(), device="cuda")
    off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    enc = batch.Encoder(len(blocks), total, sq.bound(max(sizes)))
    want = [O.tokens(b, WINDOW) for b in blocks]
    for finder in ("index", "scan"):
        toks, counts = enc.tokens(d_in, off, WINDOW, finder=finder)
        torch.cuda.synchronize()
        h_toks = toks.cpu().numpy().view(np.uint32)
        h_counts = counts.cpu().numpy()
        for k, w in enumerate(want):
            assert int(h_counts[k]) == len(w), (finder, k, sizes[k])
            got = h_toks[int(offs[k]):int(offs[k]) + len(w)]
            assert (got == w).all(), (finder, k, sizes[k])


# tile size - 1, tile size and tile size + 1 positions (+ the two bytes without a key), for one and for two tiles
TILE_EDGES = [k * TILE + d + 2 for k in (1, 2) for d in (-1, 0, 1)]


@pytest.mark.parametrize("n_bytes", [3, 4, 66] + TILE_EDGES)
def test_short_blocks_and_tile_edges(sq, batch, n_bytes):
    _check(sq, batch, [O.zipf_block(3, n_bytes)])


@pytest.mark.parametrize("n_bytes", TILE_EDGES)
def test_tile_edges_random_bytes(sq, batch, n_bytes):
    _check(sq, batch, [_random_bytes(n_bytes, n_bytes)])


def test_zeros_one_digit_takes_every_tile(sq, batch):
    _check(sq, batch, [bytes(1 << 18)])


def test_period_three(sq, batch):
    _check(sq, batch, [(b"\x07\xf3\x80" * 20000)[:50001]])


def test_uniform_random_all_digits_equally_full(sq, batch):
    _check(sq, batch, [_random_bytes(1 << 18, 18)])


def test_blocks_of_different_lengths_in_one_launch(sq, batch):
    blocks = [O.zipf_block(1, 5000), b"", b"ab", O.zipf_block(2, TILE + 2), _random_bytes(9000, 9),
              b"abc", O.zipf_block(4, 3 * TILE + 1), bytes(4099), b"abcd", O.zipf_block(6, 66)]
    _check(sq, batch, blocks)
