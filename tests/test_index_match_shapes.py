"""index_match_kernel, the shapes its page pipeline can get wrong (lz77_index.hip, tests/match_shapes.py): the indexed
finder must give the brute-force scan's tokens and the oracle's, token for token, in ONE launch per case.  A wave loads a
page's positions two pages ahead and their 16 bytes one page ahead, from clamped ranks and from min(i, n - 16), and every
lane stores -- so the cases are blocks shorter than 16 bytes and on either side of the shifted tail load, counts of one
page exactly, one rank over and two pages, a workgroup's four waves with one page each and the first rank of a second
workgroup, one ragged launch (a 40 KB block among thirty of 100..300 bytes: dozens of pages per wave, most waves of the
short blocks without a page), and the data of each path: zeros (the shared walk, 257-byte matches, the deferred own
walk), period three, random bytes (all literals), text (runs longer than 64 ranks and matches longer than 16 bytes:
walk() behind the candidate loop) and the benchmark's Zipf bytes.  Window 2^10 keeps the oracle in seconds."""
import numpy as np
import pytest

import match_shapes as shapes
import oracle_lib as O

pytestmark = pytest.mark.gpu

WINDOW = 1 << 10
CASES = shapes.cases()


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


@pytest.mark.parametrize("name", list(CASES))
def test_index_finder_is_the_scan_and_the_oracle(sq, name):
    _check(sq, CASES[name])
