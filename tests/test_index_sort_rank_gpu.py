"""index_sort_kernel, where a wrong rank can show (lz77_index.hip, sort_rank.h): a row of 64 elements is ranked by one
peer mask per lane, built from the lanes that DIFFER (one three-input operation per key bit and half of the mask, the
ballot taken of the spread bit's sign), and the first lane of every digit adds the digit's count to the wave's 16-bit
counter before the next row reads it.  A lost or doubled peer, a count in the wrong counter, or a row that read before
the write of the row before it: each moves an element inside a run of equal keys or into another run, the positions
of a run are no longer ascending, and the indexed finder stops agreeing with the brute-force scan and the oracle about
which candidate is nearest.  So the check is the one of test_index_sort_bases_gpu.py: index finder == scan finder ==
oracle, token for token, window 2^10.  The shapes: one digit in every row of two full tiles (every lane 63 peers, a
wave's counter reaches 256: an even digit, an odd one, the last of the counter row); neighbouring digits 2k and 2k+1
in one row (their counters share a 32-bit word); the first and the last digit only; rows and tiles with a ragged end,
down to a tile of one element (a lane without an element is nobody's peer); the 8 + 8 + 8 split; and all but the long
block in one launch.  What the kernel changed is the mask; its rows still read, wait, write and wait one after the
other.  The shapes with odd digits and with digits 2k and 2k+1 in one row were chosen for a variant that adds to the
32-bit word the two counters share -- built, measured, no gain, not kept ("the sort's peer
masks") -- and stay as checks of the per-row path, which whoever tries that variant again will need."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

WINDOW = 1 << 10
LARGE = (1 << 18) + 1       # the shortest block sorted by 8 + 8 + 8 bits
RAGGED = (63, 64, 65, 255, 256, 257, 4095, 4096, 4097)      # positions: n_bytes - 2


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


def _five_values(n, seed):
    return np.random.default_rng(seed).integers(0, 5, n, dtype=np.uint8).tobytes()


def _two_values(n, seed):
    return (np.random.default_rng(seed).integers(0, 2, n, dtype=np.uint8) * 0xFF).astype(np.uint8).tobytes()


# 8,194 bytes: 8,192 positions, two full tiles, every row 64 peers.  0x00: digit 0 in every pass; 0x01: digits 0x101,
# 64 and 0 (an odd digit in pass 0); 0xFF: digits 0x3FF, 127 and 127 (odd in every pass, the last counter of the row)
ONE_DIGIT = {0x00: bytes(8194), 0x01: b"\x01" * 8194, 0xFF: b"\xFF" * 8194}


@pytest.mark.parametrize("value", sorted(ONE_DIGIT))
def test_one_digit_everywhere(sq, batch, value):
    _check(sq, batch, [ONE_DIGIT[value]])


def test_neighbouring_digits_in_one_row(sq, batch):
    # pass 2: digits 0 and 1; pass 1: 0, 1, 64 and 65; pass 0: 0 .. 4 plus 256 j
    _check(sq, batch, [_five_values(8500, 11)])


def test_first_and_last_digits(sq, batch):
    _check(sq, batch, [_two_values(8500, 12)])


@pytest.mark.parametrize("positions", RAGGED)
def test_ragged_rows_and_tiles(sq, batch, positions):
    # (4097 positions: a second tile of one element)
    _check(sq, batch, [O.zipf_block(3, positions + 2), _five_values(positions + 2, positions)])


def test_8_8_8_split(sq, batch):
    _check(sq, batch, [_five_values(LARGE, 13)])


def test_one_mixed_launch(sq, batch):
    blocks = [ONE_DIGIT[0x00], ONE_DIGIT[0x01], ONE_DIGIT[0xFF], _five_values(8500, 11), _two_values(8500, 12)]
    for positions in RAGGED:
        blocks += [O.zipf_block(3, positions + 2), _five_values(positions + 2, positions)]
    _check(sq, batch, blocks)
