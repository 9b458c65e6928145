"""TEST INFRASTRUCTURE: the one-step lazy parse in plain Python, over the oracle's match finder.

L(i), D(i) = oracle_lib.match_at (the longest match at i: strict >, nearest first, 0 or 3..257; none at the
last two positions).  On the path at i:

  * L(i) >= 3, i + 1 < n and L(i + 1) > L(i): the literal data[i], go to i + 1
  * otherwise L(i) >= 3: the match (L(i), D(i)), go to i + L(i)
  * otherwise: the literal data[i], go to i + 1

lazy=False leaves the first case out: the reference's greedy step (oracle_lib.tokens).  Token words are the
ones stage 1 writes: the byte for a literal, 0x80000000 | len << 16 | dist for a match."""
import numpy as np

import oracle_lib as O

TOK_MATCH = 0x80000000
LEN_MIN = 3


def table(data: bytes, window: int):
    """(L, D) for every position; L = 0 where there is no match"""
    n = len(data)
    L = np.zeros(n, np.int64)
    D = np.zeros(n, np.int64)
    for i in range(max(n - 2, 0)):
        ln, ds = O.match_at(data, i, window)
        if ln >= LEN_MIN:
            L[i], D[i] = ln, ds
    return L, D


def parse(data: bytes, window: int, lazy: bool, tab=None):
    """-> (token words, positions that gave way to their successor, in path order)"""
    L, D = table(data, window) if tab is None else tab
    n = len(data)
    out, gave = [], []
    i = 0
    while i < n:
        li = int(L[i])
        if lazy and li >= LEN_MIN and i + 1 < n and int(L[i + 1]) > li:
            out.append(data[i])
            gave.append(i)
            i += 1
        elif li >= LEN_MIN:
            out.append(TOK_MATCH | (li << 16) | int(D[i]))
            i += li
        else:
            out.append(data[i])
            i += 1
    return np.array(out, np.uint32), gave


def stream(toks) -> bytes:
    """the payload stage 2 writes for these token words (the oracle's coder)"""
    e, comp, _ = O.encode_tokens(toks)
    assert e == 0, e
    return comp


def longest_chain(gave):
    """the longest run of consecutive positions in `gave`"""
    best = run = 0
    prev = None
    for p in gave:
        run = run + 1 if prev is not None and p == prev + 1 else 1
        best = max(best, run)
        prev = p
    return best
