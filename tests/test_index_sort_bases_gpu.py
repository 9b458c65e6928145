"""index_sort_kernel, where a wrong bucket base can show (lz77_index.hip, sort_bases.h): the kernel counts pass 0's
digit per position and derives the histograms of passes 1 and 2 from that one -- sums of its bins, put right by the
block's first two and last two bytes.  A wrong base moves a run of the sorted positions, and the indexed finder stops
agreeing with the brute-force scan and the oracle, so the check is the one of test_index_sort_shapes.py: index finder
== scan finder == oracle, token for token, window 2^10.  The shapes: lengths at which the sweep has no quad or a first
quad and a tail; end bytes that occur nowhere else in the block (every correction then moves a bin that the sum of
bins leaves wrong by one), at the head only, at the tail only, and end bytes equal to the most frequent byte; both
digit splits (10 + 7 + 7 up to 2^18 bytes, 8 + 8 + 8 beyond); bytes that differ only in the bits that move between
neighbouring digits; and blocks of all kinds in one launch (a block's derivation must not read a neighbour's bytes)."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

WINDOW = 1 << 10
LARGE = (1 << 18) + 1       # the shortest block sorted by 8 + 8 + 8 bits


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


ENDS = ("head_and_tail", "head", "tail", "most_frequent")


def _end_bytes_block(n, which, seed=5):
    """Zipf bytes clipped below 0xF0 with the first two bytes 0xFB, 0xFD and / or the last two 0xFE, 0xFF -- values
    that occur nowhere else -- or with all four end bytes equal to the body's most frequent byte"""
    b = np.minimum(np.frombuffer(O.zipf_block(seed, n), np.uint8), 0xEF).astype(np.uint8)
    if which == "most_frequent":
        b[[0, 1, n - 2, n - 1]] = np.bincount(b, minlength=256).argmax()
    if which in ("head_and_tail", "tail"):
        b[n - 2:] = (0xFE, 0xFF)
    if which in ("head_and_tail", "head"):
        b[:2] = (0xFB, 0xFD)
    return b.tobytes()


def _random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _five_values(n, seed):
    return np.random.default_rng(seed).integers(0, 5, n, dtype=np.uint8).tobytes()


# 4..7: no quad, the one-by-one tail only; 8, 9, 11, 12, 13: the first quads and their tails
@pytest.mark.parametrize("n_bytes", [4, 5, 6, 7, 8, 9, 11, 12, 13, 66])
def test_length_edges(sq, batch, n_bytes):
    _check(sq, batch, [O.zipf_block(3, n_bytes)])


@pytest.mark.parametrize("which", ENDS)
@pytest.mark.parametrize("n_bytes", [66, 4098])
def test_end_bytes_10_7_7(sq, batch, n_bytes, which):
    _check(sq, batch, [_end_bytes_block(n_bytes, which)])


@pytest.mark.parametrize("which", ENDS)
def test_end_bytes_8_8_8(sq, batch, which):
    _check(sq, batch, [_end_bytes_block(LARGE, which)])


def test_uniform_random_8_8_8(sq, batch):
    _check(sq, batch, [_random_bytes((1 << 18) + 5, 23)])


def test_neighbouring_digits(sq, batch):
    _check(sq, batch, [_five_values(5000, 7)])


def test_one_mixed_launch(sq, batch):
    blocks = [_end_bytes_block(66, "head_and_tail"), b"", O.zipf_block(3, 7), b"ab", _end_bytes_block(4098, "tail"),
              _five_values(5000, 7), b"abc", _end_bytes_block(4098, "head"), O.zipf_block(3, 13),
              _end_bytes_block(66, "most_frequent"), _random_bytes(4099, 4), O.zipf_block(3, 4)]
    _check(sq, batch, blocks)
