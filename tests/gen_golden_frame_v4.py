"""Writes tests/golden/ramp_u32.w15.b12.e4.sqzf: the SQZF version-4 frame of the `u32` ramp of the payload table
(tests/frame_writer_v4.py, 16389 bytes) at window 2^15 in blocks of 4096 bytes, shuffled as 4-byte elements, every
stream produced by the COMPILED REFERENCE (oracle/_ref/libsqz_ref.so, squeeze_compress without its header) over the
shuffled block.  Run where that library exists:  python tests/gen_golden_frame_v4.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_writer_v4 as W4  # noqa: E402
import oracle_lib as O  # noqa: E402

NAME = "ramp_u32.w15.b12.e4.sqzf"

if __name__ == "__main__":
    assert O.REF is not None, "oracle/_ref/libsqz_ref.so is missing"
    data = W4.figure_input("u32_ramp")
    streams = W4.streams_of(data, 15, 12, 4, encode=lambda s: O.ref_compress(s, 15, header=False))
    frame = W4.assemble(data, 15, 12, 4, streams)
    path = os.path.join(O.GOLD, NAME)
    with open(path, "wb") as fh:
        fh.write(frame)
    print(path, len(frame), "bytes")
