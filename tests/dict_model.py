"""TEST INFRASTRUCTURE: blocks coded under a shared dictionary, as a model over the oracle's match finder.

The stream of a block B under a dictionary Dct is what the reference's encoder writes for the bytes Dct || B when it
starts, with fresh trees, at position D = len(Dct).  Two steps, nothing new under oracle/:

  * a greedy walk (and the lazy one of tests/lazy_model.py) over L(i), D(i) = oracle_lib.match_at(Dct + B, D + i,
    window): distances 1 .. min(D + i, window - 1), nearest first, strict >, lengths up to min(len(B) - i, 257); a
    source may begin in the dictionary and run on into the block
  * the token words through oracle_lib.encode_tokens (stage 2 of the restatement)

and, for the decode side, a token expander in plain Python that takes a history.  With Dct = b"" the stream is
oracle_lib.encode(B, ..., header=False) byte for byte (tests/test_dict_cpu.py)."""
import numpy as np

import lazy_model as LM
import oracle_lib as O

TOK_MATCH = LM.TOK_MATCH
LEN_MIN = LM.LEN_MIN


def table(dct: bytes, block: bytes, window: int):
    """(L, D) for every position of the block; L = 0 where there is no match"""
    n, d = len(block), len(dct)
    both = dct + block
    L = np.zeros(n, np.int64)
    D = np.zeros(n, np.int64)
    for i in range(max(n - 2, 0)):
        ln, ds = O.match_at(both, d + i, window)
        if ln >= LEN_MIN:
            L[i], D[i] = ln, ds
    return L, D


def tokens(dct: bytes, block: bytes, window: int, lazy: bool = False, tab=None):
    """the token words of the block under the dictionary"""
    if tab is None:
        tab = table(dct, block, window)
    return LM.parse(block, window, lazy, tab)[0]


def stream(dct: bytes, block: bytes, window: int, lazy: bool = False) -> bytes:
    return LM.stream(tokens(dct, block, window, lazy))


def expand(toks, history: bytes = b"") -> bytes:
    """token words -> bytes, with `history` standing in front of the output (byte-serial: a copy may overlap itself)"""
    buf = bytearray(history)
    for w in (int(t) for t in toks):
        if w & TOK_MATCH:
            ln, ds = (w >> 16) & 0x1FF, w & 0x7FFF
            assert 1 <= ds <= len(buf), (ds, len(buf))
            for _ in range(ln):
                buf.append(buf[-ds])
        else:
            buf.append(w)
    return bytes(buf[len(history):])


def sources(toks, d: int):
    """per match token: (block position o, length, distance, first source position in Dct || B minus d) -- a
    negative last entry is a source that starts in the dictionary"""
    out, o = [], 0
    for w in (int(t) for t in toks):
        if w & TOK_MATCH:
            ln, ds = (w >> 16) & 0x1FF, w & 0x7FFF
            out.append((o, ln, ds, o - ds))
            o += ln
        else:
            o += 1
    return out


# ---- the inputs of the emulator and GPU tests ---------------------------------------------------------------
# The corners of the feature do not occur in ordinary text (a 4 KB block of laozi.txt has hundreds of matches into
# the dictionary, none that straddles its end and none whose source starts in its last two bytes), so they are
# planted, and corners() says from the model's tokens which ones are on the path: the tests assert that before they
# compare anything.
def corners(toks, d: int) -> set:
    out = set()
    for o, ln, ds, s in sources(toks, d):
        if s >= 0:
            continue
        out.add("dict")
        if s == -1:
            out.add("source_at_D-1")
        if s == -2:
            out.add("source_at_D-2")
        if s + ln > 0:
            out.add("straddle")
        if ds < ln:
            out.add("periodic_from_dict")
        if o == 0:
            out.add("first_token")
        if ln == 257:
            out.add("len_257")
    return out


def dict_only_length(dct: bytes, block: bytes, i: int, window: int) -> int:
    """the longest match at block position i among the sources that START in the dictionary (brute force)"""
    d, both = len(dct), dct + block
    cap = min(len(block) - i, 257)
    best = 0
    for q in range(max(d + i - (window - 1), 0), d):
        k = 0
        while k < cap and both[q + k] == block[i + k]:
            k += 1
        best = max(best, k)
    return best


def ties_kept_in_block(dct: bytes, block: bytes, window: int, toks) -> list:
    """on-path matches with an in-block source where the dictionary holds one of exactly the same length"""
    return [o for o, ln, ds, s in sources(toks, len(dct)) if s >= 0 and dict_only_length(dct, block, o, window) == ln]


def cases(lao: bytes, con: bytes):
    """[(name, window, dictionary, [blocks], corners that must be on the greedy path of block 0)]"""
    tiny = [b"", b"a", b"ab", b"abc"]
    return [
        # two straddles, a source in the last two bytes, a periodic copy that starts in the dictionary
        ("tail", 1 << 15, lao[:4000] + b"QZ",
         [b"QZQZQZQZQZQZ" + lao[4000:4500] + lao[3990:4000] + b"QZQZx"] + tiny + [lao[4500:4600]],
         {"source_at_D-2", "straddle", "periodic_from_dict", "first_token"}),
        ("first", 1 << 15, lao[:3000] + b"abcde", [b"abcde" * 4 + lao[3000:3300], lao[3300:3400]],
         {"first_token", "periodic_from_dict", "straddle"}),
        # Dct[D-1] = 'x' and the block starts "yzxyzxyz": position 2 finds x,y,z,... at distance 3 = source D-1
        ("last_byte", 1 << 15, lao[:500] + b"x", [b"yzxyzxyzxyz" + lao[500:700]], {"source_at_D-1"}),
        # 300 bytes of the dictionary again: a match of 257; the marker's second copy in the block ties with the dictionary's
        ("long_and_tie", 1 << 15, lao[:2000] + b"#HELLOWORLD1#",
         [lao[100:400] + b"@HELLOWORLD2@" + lao[2000:2200] + b"%HELLOWORLD3%" + lao[2200:2250]], {"len_257", "first_token"}),
        # window 2^10, D = 1023: position i reaches dictionary positions >= i only, later ones lose its front
        # (the block's position 1 is the dictionary's position 0: distance 1024, one too far)
        ("w10", 1 << 10, lao[:1023], [lao[0:1] + lao[0:300] + lao[1023:1800], lao[2000:2100]] + tiny, {"dict"}),
        # window 2^15, D = 32767, blocks of 4,096 and 5,000 bytes
        ("w15_full", 1 << 15, con[:32767], [con[30000:34096], lao[:5000]], {"len_257", "first_token"}),
        # dictionaries whose index is empty or nearly so
        ("D1", 1 << 15, b"t", [b"tttttttt the way" + lao[:200]] + tiny, {"source_at_D-1", "first_token"}),
        ("D2", 1 << 15, b"ab", [b"ababab" + lao[:200], b"b"], {"source_at_D-2", "first_token"}),
        ("D3", 1 << 15, b"the", [b"the way the way" + lao[:200], b"th"], {"first_token"}),
    ]
