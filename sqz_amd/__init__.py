"""sqz_amd -- MI355X-native LZ77 + adaptive-Huffman encode/decode path of sqz.

The product is libsqz_amd.so (hand-written HIP for gfx950 behind the C ABI of
include/sqz/sqz.h).  This package is the thin host side: ctypes binding,
a mirror of the reference's codec interface, the device-resident batch path and
the multi-GPU block sharding.
"""
from .codec import (SqzError, bound, compress, decompress, device_info,  # noqa: F401
                    file_words, MIN_WIN_BITS, MAX_WIN_BITS)

__all__ = ["SqzError", "bound", "compress", "decompress", "device_info", "file_words",
           "MIN_WIN_BITS", "MAX_WIN_BITS", "compress_frame", "decompress_frame", "frame_info", "read_range",
           "frame_blocks", "frame_bound", "gather_frame", "update_frame", "append_frame", "shuffle_blocks",
           "frames_bound", "encode_frames", "decode_frames", "compress_frames", "decompress_frames"]

_FRAME = ("compress_frame", "decompress_frame", "frame_info", "read_range", "frame_blocks", "frame_bound", "gather_frame", "update_frame",
          "append_frame", "shuffle_blocks", "frames_bound", "encode_frames", "decode_frames", "compress_frames",
          "decompress_frames")


def __getattr__(name):
    # SQZF frames (sqz_amd/frame.py), loaded on first use so that `python -m sqz_amd.frame` runs it once
    if name in _FRAME:
        from . import frame
        return getattr(frame, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
