"""The block shapes at which index_match_kernel's page pipeline can go wrong (sqz_amd/csrc/lz77_index.hip), shared by
tests/test_index_match_emu.py (CPU wave emulator) and tests/test_index_match_shapes.py (GPU).  A block of n bytes has
count = n - 2 positions with a 3-byte prefix; a page is 64 consecutive ranks, a workgroup has four waves.

Not a test module: the two files import it."""
import numpy as np

import oracle_lib as O

SHORT = (3, 4, 15, 16, 17, 18, 19)       # the sub-16-byte path, and the shifted tail load on either side of its edge
PAGE_EDGES = (65, 66, 67, 129, 130)      # count = 63, 64, 65, 127, 128: one page exactly, one rank over, two pages
GROUP_EDGES = (258, 1026)                # a workgroup's four waves with one page each; the first rank of a second workgroup


def _random(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def by_length(lengths, seed):
    """Zipf bytes of the given lengths (the benchmark's own data), one block each"""
    return [O.zipf_block(seed + k, n) for k, n in enumerate(lengths)]


def ragged():
    """one 40 KB block among thirty of 100..300 bytes: match_groups follows the average, so the long block's waves
    own dozens of pages each (the double buffer runs long) and most waves of the short blocks own no page"""
    rng = np.random.default_rng(77)
    sizes = [int(s) for s in rng.integers(100, 301, 30)]
    blocks = [O.zipf_block(40 + k, n) for k, n in enumerate(sizes)]
    blocks.insert(11, O.zipf_block(39, 40 * 1024))
    return blocks


def cases():
    """name -> blocks of ONE launch"""
    return {
        "short": by_length(SHORT, 100) + [bytes(n) for n in SHORT] + [_random(3, n) for n in SHORT],
        "page_edges": by_length(PAGE_EDGES, 200) + [bytes(n) for n in PAGE_EDGES],
        "group_edges": by_length(GROUP_EDGES, 300) + [bytes(n) for n in GROUP_EDGES],
        "ragged": ragged(),
        "zeros": [bytes(5000)],                                  # whole wave in one run, 257-byte matches, the deferred own walk
        "period3": [(b"\x07\xf3\x80" * 1700)[:5000]],            # long matches that begin off the page grid
        "random": [_random(5, 4099)],                            # all literals
        "text": [O.corpus("confucius.txt")[:8192]],              # runs longer than 64 ranks, matches longer than 16 bytes: walk()
        "zipf": [O.zipf_block(9, 4099)],                         # the benchmark's data at a size that is a multiple of nothing
    }
