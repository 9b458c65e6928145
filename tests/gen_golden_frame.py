"""Writes tests/golden/laozi.txt.w15.b12.sqzf: the SQZF frame of tests/corpus/laozi.txt at window 2^15 in blocks
of 4096 bytes, every stream produced by the COMPILED REFERENCE (oracle/_ref/libsqz_ref.so, squeeze_compress
without its header).  Run where that library exists:  python tests/gen_golden_frame.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_writer as W  # noqa: E402
import oracle_lib as O  # noqa: E402

if __name__ == "__main__":
    assert O.REF is not None, "oracle/_ref/libsqz_ref.so is missing"
    frame = W.write_frame(O.corpus("laozi.txt"), 15, 12, encode=lambda blk: O.ref_compress(blk, 15, header=False))
    path = os.path.join(O.GOLD, "laozi.txt.w15.b12.sqzf")
    with open(path, "wb") as fh:
        fh.write(frame)
    print(path, len(frame), "bytes")
