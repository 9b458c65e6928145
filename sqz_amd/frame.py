"""SQZF frames: one checksummed, seekable artifact for one large buffer (include/sqz/sqz.h).

Host flavour (bytes in, bytes out) and a device flavour over torch tensors in the style of batch.py.
Every byte of codec and checksum work happens in libsqz_amd.so; nothing is computed here.

    python -m sqz_amd.frame c IN OUT [--win-bits 15] [--block-bits 18] [--store] [--lazy] [--dict FILE] [--shuffle N]
                                                                           compress a file
    python -m sqz_amd.frame d IN OUT [--dict FILE]                         decompress one
    python -m sqz_amd.frame a FRAME IN OUT [--lazy] [--dict FILE]          append IN's bytes to FRAME (append_frame)
    python -m sqz_amd.frame info IN                                        describe one
    python -m sqz_amd.frame blocks IN                                      one line per block

store=True / --store writes version 2: a block whose stream is not smaller than its content is stored as it is.
parse="lazy" / --lazy encodes with one position of look-ahead (codec.parse_code): smaller streams in the same frame
format, read by every reader; the default, "greedy", is the reference's parse.
dictionary=bytes / --dict FILE writes version 3: every block may reach back into the dictionary (1 .. window - 1
bytes) as if it stood in front of the block.  The frame records the dictionary's length and CRC-32, not the
dictionary: the reader brings the same bytes (anything else is EILSEQ).  For frames of small blocks of text; it can
make an executable larger (README).
shuffle=2|4|8 / --shuffle N writes version 4: every block is byte-shuffled in front of the encoder -- all first bytes
of its N-byte elements, then all second bytes, and so on -- which is what arrays of numbers want (README has the
figures; noise gains nothing and a few inputs lose a little, so it is opt-in).  The readers pick the version up from
the header.  Not together with a dictionary; gather, update and append do not take version 4 yet.
The batch calls (frames_bound, encode_frames, compress_frames) take shuffle= as well: one element size for every frame
or a sequence with one per frame, 0 for a frame that is not shuffled -- a set of tensors in one launch chain; and
decode_frames / decompress_frames take versions 1, 2 and 4 in any mix with shuffled=True.  The defaults are the calls
as they were, which write versions 1 and 2 and refuse a version-4 frame.
"""
import collections
import ctypes as C
import errno

from . import _native as N
from .codec import MAX_DICT_BYTES, PARSE_LAZY, SqzError, _raise, dict_bytes, parse_code

HEADER_BYTES = 32
FRAME_STORED = 1            # SQZ_FRAME_STORED
FRAME_DICT = 2              # SQZ_FRAME_DICT
FRAME_SHUFFLE = 4           # SQZ_FRAME_SHUFFLE


def shuffle_code(shuffle) -> int:
    """shuffle= as the element size of a version-4 frame: 0 (none), 2, 4 or 8; anything else is ValueError"""
    if isinstance(shuffle, bool) or shuffle not in (0, 2, 4, 8):
        raise ValueError(f"shuffle must be 0, 2, 4 or 8, not {shuffle!r}")
    return int(shuffle)


def _shuffle_arg(shuffle, dictionary) -> int:
    e = shuffle_code(shuffle)
    if e != 0 and dictionary is not None:
        raise ValueError("shuffle and dictionary do not go together: a frame is version 3 or version 4")
    return e


def _no_version_4(info: dict, who: str):
    if info["version"] == 4:
        raise ValueError(f"{who}: a version-4 (shuffled) frame is not supported here yet; decode and encode it again")


def _flags(store: bool) -> int:
    return FRAME_STORED if store else 0


def frame_bound(nbytes: int, block_bits: int = 18, store: bool = False, dictionary: bool = False,
                shuffle: int = 0) -> int:
    """worst-case size of the frame of `nbytes` bytes of content"""
    if shuffle_code(shuffle) != 0:
        return int(N.lib().sqz_frame_bound_shuf(nbytes, block_bits, _flags(store) | FRAME_SHUFFLE))
    if dictionary:
        return int(N.lib().sqz_frame_bound_dict(nbytes, block_bits, _flags(store) | FRAME_DICT))
    return int(N.lib().sqz_frame_bound_ex(nbytes, block_bits, _flags(store)))


class _FrameInfo(dict):
    """frame_info()'s result.  A version-3 header has a dictionary record, and its two fields are keys; versions 1
    and 2 have none: there the fields read as 0 without being keys, so the dict still equals the header's own
    fields."""

    def __missing__(self, key):
        if key in ("dict_bytes", "dict_crc", "elem_bytes"):
            return 0
        raise KeyError(key)


def frame_info(frame) -> dict:
    """The header's fields (sqz_frame_info), checked; with the index in reach, that too.
    dict_bytes / dict_crc: the record of a version-3 frame (0 while it is not in reach).  For versions 1 and 2, which
    have no record, info["dict_bytes"] and info["dict_crc"] READ as 0 but are NOT keys of the result: `in`, .get(),
    iteration and the `info` tool show them for a version-3 frame only, so that the result of an older frame keeps
    exactly the header's own eight fields.  Test the version (info["version"] == 3), not the key.
    elem_bytes: the record of a version-4 frame, in the same way a key for version 4 only (0 while it is not in reach).
    Host code: no device is touched."""
    frame = bytes(frame)
    fi = N.FrameInfo()
    _raise(N.lib().sqz_frame_info(frame, len(frame), C.byref(fi)), "sqz_frame_info")
    info = _FrameInfo({k: int(getattr(fi, k)) for k, _ in N.FrameInfo._fields_ if k != "reserved"})
    if fi.version == 3:
        nb, crc = C.c_uint32(0), C.c_uint32(0)
        if len(frame) >= fi.payload_off:
            _raise(N.lib().sqz_frame_dict(frame, len(frame), C.byref(nb), C.byref(crc)), "sqz_frame_dict")
        info["dict_bytes"], info["dict_crc"] = nb.value, crc.value
    if fi.version == 4:
        eb = C.c_uint32(0)
        if len(frame) >= fi.payload_off:
            _raise(N.lib().sqz_frame_elem(frame, len(frame), C.byref(eb)), "sqz_frame_elem")
        info["elem_bytes"] = eb.value
    return info


def frame_blocks(frame) -> list:
    """One dict per block (sqz_frame_blocks): payload_off (from the start of the frame), payload_bytes,
    content_bytes, content_crc, stored.  Host code: needs header and index, no device is touched."""
    frame = bytes(frame)
    n = frame_info(frame)["n_blocks"]
    out = (N.FrameBlock * max(n, 1))()
    _raise(N.lib().sqz_frame_blocks(frame, len(frame), 0, n, out), "sqz_frame_blocks")
    return [{k: int(getattr(out[b], k)) for k, _ in N.FrameBlock._fields_} for b in range(n)]


def compress_frame(data, win_bits: int = 15, block_bits: int = 18, store: bool = False,
                   parse: str = "greedy", dictionary=None, shuffle: int = 0) -> bytes:
    lazy = parse_code(parse) == PARSE_LAZY
    elem = _shuffle_arg(shuffle, dictionary)
    dct = dict_bytes(dictionary, 1 << win_bits) if dictionary is not None else None
    data = bytes(data)
    cap = frame_bound(len(data), block_bits, store, dct is not None, elem)
    if cap == 0:
        raise SqzError(errno.EINVAL, "sqz_frame_compress: block_bits out of range")
    out = bytearray(cap)
    n = C.c_uint64(0)
    dst = (C.c_uint8 * cap).from_buffer(out)
    if elem != 0:
        _raise(N.lib().sqz_frame_compress_shuf(data, len(data), win_bits, block_bits, _flags(store) | FRAME_SHUFFLE,
                                               parse_code(parse), elem, dst, cap, C.byref(n)), "sqz_frame_compress_shuf")
    elif dct is not None:
        _raise(N.lib().sqz_frame_compress_dict(data, len(data), win_bits, block_bits, _flags(store), parse_code(parse),
                                               dct, len(dct), dst, cap, C.byref(n)), "sqz_frame_compress_dict")
    elif lazy:
        _raise(N.lib().sqz_frame_compress_parse(data, len(data), win_bits, block_bits, _flags(store), PARSE_LAZY, dst,
                                                cap, C.byref(n)), "sqz_frame_compress_parse")
    else:
        _raise(N.lib().sqz_frame_compress_ex(data, len(data), win_bits, block_bits, _flags(store), dst, cap,
                                             C.byref(n)), "sqz_frame_compress_ex")
    del dst
    return bytes(out[:n.value])


def decompress_frame(frame, return_errors: bool = False, dictionary=None):
    """The content of a frame.  A block that fails raises SqzError with the first errno; its attribute
    block_errors lists every block's.  return_errors=True returns (bytes, block_errors) instead: good
    blocks are delivered, bad ones hold whatever the decoder produced.  dictionary: what a version-3 frame was
    written with (a wrong one is EILSEQ; a version-3 frame without one, or another frame with one, EINVAL)."""
    dct = dict_bytes(dictionary) if dictionary is not None else None
    frame = bytes(frame)
    fi = frame_info(frame[:HEADER_BYTES])
    out = bytearray(max(fi["content_bytes"], 1))
    dst = (C.c_uint8 * len(out)).from_buffer(out)
    errs = (C.c_int32 * max(fi["n_blocks"], 1))()
    n = C.c_uint64(0)
    if dct is not None:
        rc = N.lib().sqz_frame_decompress_dict(frame, len(frame), dct, len(dct), dst, fi["content_bytes"], C.byref(n),
                                               errs)
    elif fi["version"] == 4:
        rc = N.lib().sqz_frame_decompress_shuf(frame, len(frame), dst, fi["content_bytes"], C.byref(n), errs)
    else:
        rc = N.lib().sqz_frame_decompress(frame, len(frame), dst, fi["content_bytes"], C.byref(n), errs)
    del dst
    block_errors = list(errs)[:fi["n_blocks"]]
    if return_errors and (rc == 0 or any(block_errors)):
        return bytes(out[:fi["content_bytes"]]), block_errors
    if rc != 0:
        e = SqzError(rc, f"sqz_frame_decompress: {errno.errorcode.get(rc, rc)}")
        e.block_errors = block_errors
        raise e
    return bytes(out[:n.value])


def read_range(frame, offset: int, length: int, dictionary=None) -> bytes:
    """content[offset : offset + length]: only the covering blocks are uploaded, decoded and verified.
    dictionary: as for decompress_frame."""
    dct = dict_bytes(dictionary) if dictionary is not None else None
    frame = bytes(frame)
    fi = frame_info(frame[:HEADER_BYTES])
    content = fi["content_bytes"]
    out = bytearray(max(min(length, content), 1))            # a range that leaves the content is refused below
    dst = (C.c_uint8 * len(out)).from_buffer(out)
    if dct is not None:
        rc = N.lib().sqz_frame_read_dict(frame, len(frame), dct, len(dct), offset, length, dst)
    elif fi["version"] == 4:
        rc = N.lib().sqz_frame_read_shuf(frame, len(frame), offset, length, dst)
    else:
        rc = N.lib().sqz_frame_read(frame, len(frame), offset, length, dst)
    del dst
    _raise(rc, "sqz_frame_read_dict" if dct is not None else "sqz_frame_read")
    return bytes(out[:length])


# ---- device flavour (torch tensors hold the HBM) ------------------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def crc32_blocks(d_in, in_off, crc=None):
    """zlib.crc32 of n ragged byte ranges of a uint8 tensor: in_off int64[n + 1] -> int32/uint32[n] on the device"""
    import torch
    n = in_off.numel() - 1
    if crc is None:
        crc = torch.zeros(max(n, 1), dtype=torch.int32, device=d_in.device)
    _raise(N.lib().sqz_hip_crc32_blocks(_ptr(d_in), _ptr(in_off), n, _ptr(crc), _stream()), "sqz_hip_crc32_blocks")
    return crc[:n]


def shuffle_blocks(d_in, offsets, elem_bytes: int, inverse: bool = False, d_out=None):
    """The byte shuffle of version 4 over n ragged ranges of a uint8 tensor: offsets int64[n + 1] on the device, range b
    = d_in[offsets[b] : offsets[b + 1]], each transposed on its own into the same place of d_out (a tensor of d_in's
    size, made when not given; it must not overlap d_in): all first bytes of its elem_bytes-wide elements, then all
    second bytes, ..., the tail bytes behind; inverse=True undoes it.  Bytes outside every range are not written.
    Enqueues and returns d_out."""
    import torch
    if elem_bytes not in (2, 4, 8):
        raise ValueError(f"elem_bytes must be 2, 4 or 8, not {elem_bytes!r}")
    if d_in.dtype != torch.uint8 or d_in.dim() != 1 or offsets.dtype != torch.int64 or offsets.dim() != 1:
        raise ValueError("shuffle_blocks: a one-dimensional uint8 tensor and int64 offsets")
    if d_out is None:
        d_out = torch.empty_like(d_in)
    elif d_out.dtype != torch.uint8 or d_out.numel() < d_in.numel():
        raise ValueError("shuffle_blocks: d_out must be a uint8 tensor of d_in's size")
    n = max(offsets.numel() - 1, 0)
    _raise(N.lib().sqz_hip_shuffle_blocks(_ptr(d_in), _ptr(offsets), n, elem_bytes, 1 if inverse else 0, _ptr(d_out),
                                          _stream()), "sqz_hip_shuffle_blocks")
    return d_out


def _info_dev(d_frame):
    """frame_info() of a device-resident frame: one 32-byte copy, and for version 4 the record's 8 bytes behind the
    index, which say what the elements are"""
    info = frame_info(d_frame[:HEADER_BYTES].cpu().numpy().tobytes())
    if info["version"] == 4:
        at = HEADER_BYTES + 8 * info["n_blocks"]
        if d_frame.numel() >= at + 8:
            info["elem_bytes"] = int.from_bytes(d_frame[at:at + 4].cpu().numpy().tobytes(), "little")
    return info


def _dict_dev(dictionary, window, device):
    """A shared dictionary on the device, its length checked before anything native is called: bytes-like, or a
    uint8 tensor that is there already (used as it is: the caller keeps it alive until the stream has passed).
    A tensor made here comes from torch's allocator on the current stream, which does not hand its memory to
    another stream while work enqueued on this one may still read it."""
    import torch
    if isinstance(dictionary, torch.Tensor):
        if dictionary.dtype != torch.uint8 or dictionary.dim() != 1:
            raise ValueError("dictionary tensor must be one-dimensional uint8")
        most = MAX_DICT_BYTES if window is None else min(window - 1, MAX_DICT_BYTES)
        if not 1 <= dictionary.numel() <= most:
            raise ValueError(f"dictionary must be 1 .. {most} bytes, not {dictionary.numel()}")
        return dictionary.contiguous().to(device)
    d = dict_bytes(dictionary, window)
    return torch.frombuffer(bytearray(d), dtype=torch.uint8).to(device)


class FrameEncoder:
    """Reusable device buffers for frames of up to `content_bytes` bytes at (win_bits, block_bits).
    encode() enqueues and returns; frame_bytes / status / err are device tensors to read after a synchronise.
    dictionary (bytes-like or a uint8 device tensor of 1 .. window - 1 bytes): version-3 frames, byte for byte
    compress_frame(..., dictionary=)'s; it is kept on the device for the encoder's life.
    shuffle (2, 4 or 8; not with a dictionary): version-4 frames, byte for byte compress_frame(..., shuffle=)'s."""

    def __init__(self, content_bytes: int, win_bits: int = 15, block_bits: int = 18, capacity: int = None,
                 device="cuda", store: bool = False, parse: str = "greedy", dictionary=None, shuffle: int = 0):
        import torch
        self.parse = parse_code(parse)
        self.elem = _shuffle_arg(shuffle, dictionary)
        L = N.lib()
        self.win_bits, self.block_bits, self.content_bytes = win_bits, block_bits, content_bytes
        self.flags = _flags(store)
        self.dictionary = _dict_dev(dictionary, 1 << win_bits, device) if dictionary is not None else None
        if capacity is None:
            capacity = frame_bound(content_bytes, block_bits, store, self.dictionary is not None, self.elem)
        self.capacity = capacity
        self.n_blocks = (content_bytes + (1 << block_bits) - 1) >> block_bits
        self.frame = torch.empty(max(self.capacity, 16), dtype=torch.uint8, device=device)
        self.frame_bytes = torch.zeros(1, dtype=torch.int64, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.err = torch.zeros(max(self.n_blocks, 1), dtype=torch.int32, device=device)
        if self.elem != 0:
            self.scratch_bytes = int(L.sqz_hip_frame_scratch_bytes_shuf(content_bytes, block_bits, 1, self.flags))
        elif self.dictionary is not None:
            self.scratch_bytes = int(L.sqz_hip_frame_scratch_bytes_dict(content_bytes, block_bits, 1, self.flags,
                                                                        self.dictionary.numel()))
        else:
            self.scratch_bytes = int(L.sqz_hip_frame_scratch_bytes_ex(content_bytes, block_bits, 1, self.flags))
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=device)

    def encode(self, d_in, content_bytes: int = None):
        nbytes = d_in.numel() if content_bytes is None else content_bytes
        if nbytes > self.content_bytes:
            raise SqzError(errno.E2BIG, "FrameEncoder: more content than the buffers were made for")
        if self.elem != 0:
            _raise(N.lib().sqz_hip_frame_encode_shuf(
                _ptr(d_in), nbytes, self.win_bits, self.block_bits, self.flags | FRAME_SHUFFLE, self.parse, self.elem,
                _ptr(self.frame), self.capacity, _ptr(self.frame_bytes), _ptr(self.status), _ptr(self.err),
                _ptr(self.scratch), self.scratch_bytes, _stream()), "sqz_hip_frame_encode_shuf")
            return self.frame, self.frame_bytes, self.status, self.err
        if self.dictionary is not None:
            _raise(N.lib().sqz_hip_frame_encode_dict(
                _ptr(d_in), nbytes, self.win_bits, self.block_bits, self.flags | FRAME_DICT, self.parse,
                _ptr(self.dictionary), self.dictionary.numel(), _ptr(self.frame), self.capacity,
                _ptr(self.frame_bytes), _ptr(self.status), _ptr(self.err), _ptr(self.scratch), self.scratch_bytes,
                _stream()), "sqz_hip_frame_encode_dict")
            return self.frame, self.frame_bytes, self.status, self.err
        if self.parse == PARSE_LAZY:
            _raise(N.lib().sqz_hip_frame_encode_parse(
                _ptr(d_in), nbytes, self.win_bits, self.block_bits, self.flags, self.parse, _ptr(self.frame),
                self.capacity, _ptr(self.frame_bytes), _ptr(self.status), _ptr(self.err), _ptr(self.scratch),
                self.scratch_bytes, _stream()), "sqz_hip_frame_encode_parse")
            return self.frame, self.frame_bytes, self.status, self.err
        _raise(N.lib().sqz_hip_frame_encode_ex(
            _ptr(d_in), nbytes, self.win_bits, self.block_bits, self.flags, _ptr(self.frame), self.capacity,
            _ptr(self.frame_bytes), _ptr(self.status), _ptr(self.err), _ptr(self.scratch), self.scratch_bytes,
            _stream()), "sqz_hip_frame_encode_ex")
        return self.frame, self.frame_bytes, self.status, self.err

    def result(self) -> bytes:
        """synchronise and fetch the frame of the last encode(); raises on a frame-level status"""
        import torch
        torch.cuda.synchronize()
        _raise(int(self.status.item()), "sqz_hip_frame_encode_ex (status)")
        return self.frame[:int(self.frame_bytes.item())].cpu().numpy().tobytes()


_decode_scratch = {}


def _scratch_for(device, need: int):
    key = str(device)
    scratch = _decode_scratch.get(key)
    if scratch is None or scratch.numel() < need:
        import torch
        scratch = torch.empty(need, dtype=torch.uint8, device=device)
        _decode_scratch[key] = scratch
    return scratch


def decode_frame(d_frame, d_out, info: dict = None, err=None, status=None, scratch=None, dictionary=None):
    """A device-resident frame into the caller's uint8 tensor.  `info` = frame_info() of the header (fetched
    with one 32-byte copy when not given).  Enqueues and returns (err int32[n_blocks], status int32[1]).
    dictionary (bytes-like or a uint8 device tensor): what a version-3 frame was written with; a wrong one is status
    EILSEQ with nothing written, a frame of version 1 or 2 with one EINVAL.  Without one the call knows versions 1
    and 2 and refuses a version-3 frame (status EINVAL).  A version-4 frame is decoded by what `info` says about its
    elements (info["elem_bytes"]; a second small copy fetches the record when `info` is not given)."""
    import torch
    L = N.lib()
    if info is None:
        info = _info_dev(d_frame)
    n, content = info["n_blocks"], info["content_bytes"]
    if d_out.numel() < content:
        raise SqzError(errno.E2BIG, "decode_frame: d_out is smaller than the content")
    d = _dict_dev(dictionary, 1 << info["win_bits"], d_out.device) if dictionary is not None else None
    if err is None:
        err = torch.zeros(max(n, 1), dtype=torch.int32, device=d_out.device)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=d_out.device)
    if d is not None:
        if scratch is None:
            scratch = _scratch_for(d_out.device, int(L.sqz_hip_frame_scratch_bytes_dict(
                content, info["block_bytes"].bit_length() - 1, 0, FRAME_DICT, d.numel())))
        _raise(L.sqz_hip_frame_decode_dict(_ptr(d_frame), d_frame.numel(), n, content, _ptr(d), d.numel(), _ptr(d_out),
                                           _ptr(err), _ptr(status), _ptr(scratch), scratch.numel(), _stream()),
               "sqz_hip_frame_decode_dict")
        return err[:n], status
    if info["version"] == 4 and dictionary is None:
        bits = info["block_bytes"].bit_length() - 1
        if scratch is None:
            scratch = _scratch_for(d_out.device, int(L.sqz_hip_frame_scratch_bytes_shuf(content, bits, 0, FRAME_SHUFFLE)))
        _raise(L.sqz_hip_frame_decode_shuf(_ptr(d_frame), d_frame.numel(), n, content, info["elem_bytes"], _ptr(d_out),
                                           _ptr(err), _ptr(status), _ptr(scratch), scratch.numel(), _stream()),
               "sqz_hip_frame_decode_shuf")
        return err[:n], status
    need = int(L.sqz_hip_frame_scratch_bytes(content, info["block_bytes"].bit_length() - 1, 0))
    if scratch is None:
        scratch = _scratch_for(d_out.device, need)
    _raise(L.sqz_hip_frame_decode(_ptr(d_frame), d_frame.numel(), n, content, _ptr(d_out), _ptr(err), _ptr(status),
                                  _ptr(scratch), scratch.numel(), _stream()), "sqz_hip_frame_decode")
    return err[:n], status


def read_frame(d_frame, offset: int, length: int, d_out=None, info: dict = None, dictionary=None, err=None,
               status=None, scratch=None):
    """content[offset : offset + length] of a device-resident frame into d_out (uint8, made when not given): only
    the covering blocks are decoded, into the scratch, and verified.  `info` as for decode_frame; dictionary: as
    for decode_frame, needed for a version-3 frame.  Enqueues and returns (d_out[:length], err int32[covering
    blocks], status int32[1]): d_out holds the range when status is 0 after a synchronise and is untouched
    otherwise.  A range that leaves the content raises EINVAL here.  Version 4: as for decode_frame."""
    import torch
    L = N.lib()
    if info is None:
        info = _info_dev(d_frame)
    n, content, bits = info["n_blocks"], info["content_bytes"], info["block_bytes"].bit_length() - 1
    device = d_frame.device
    d = _dict_dev(dictionary, 1 << info["win_bits"], device) if dictionary is not None else None
    if d_out is None:
        d_out = torch.empty(max(length, 1), dtype=torch.uint8, device=device)
    elif d_out.numel() < length:
        raise SqzError(errno.E2BIG, "read_frame: d_out is smaller than the range")
    covering = ((offset + length - 1) >> bits) - (offset >> bits) + 1 if length > 0 else 0
    if err is None:
        err = torch.zeros(max(covering, 1), dtype=torch.int32, device=device)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=device)
    if info["version"] == 4 and d is None:
        if scratch is None:
            scratch = _scratch_for(device, int(L.sqz_hip_frame_read_scratch_bytes_shuf(length, bits)))
        _raise(L.sqz_hip_frame_read_shuf(_ptr(d_frame), d_frame.numel(), n, content, bits, info["elem_bytes"], offset,
                                         length, _ptr(d_out), _ptr(err), _ptr(status), _ptr(scratch), scratch.numel(),
                                         _stream()), "sqz_hip_frame_read_shuf")
        return d_out[:length], err[:covering], status
    if scratch is None:
        scratch = _scratch_for(device, int(L.sqz_hip_frame_read_scratch_bytes(length, bits)))
    if d is not None:
        _raise(L.sqz_hip_frame_read_dict(_ptr(d_frame), d_frame.numel(), n, content, bits, offset, length, _ptr(d),
                                         d.numel(), _ptr(d_out), _ptr(err), _ptr(status), _ptr(scratch),
                                         scratch.numel(), _stream()), "sqz_hip_frame_read_dict")
    else:
        _raise(L.sqz_hip_frame_read(_ptr(d_frame), d_frame.numel(), n, content, bits, offset, length, _ptr(d_out),
                                    _ptr(err), _ptr(status), _ptr(scratch), scratch.numel(), _stream()),
               "sqz_hip_frame_read")
    return d_out[:length], err[:covering], status


def _ranges_dev(values, device, what, who="gather_frame"):
    """a list of offsets or lengths as a uint64 device tensor's bits: (tensor, host list or None); `who` names the
    caller in the errors"""
    import torch
    if isinstance(values, torch.Tensor):
        if values.dim() != 1 or values.dtype not in (torch.int64, torch.uint64):
            raise ValueError(f"{who}: {what} must be a one-dimensional int64 or uint64 tensor")
        return values.contiguous().to(device), None
    host = [int(v) for v in values]
    if any(v < 0 or v >> 64 for v in host):
        raise ValueError(f"{who}: {what} must be 0 .. 2^64 - 1")
    signed = [v - (1 << 64) if v >> 63 else v for v in host]
    return torch.tensor(signed, dtype=torch.int64, device=device), host


def gather_bound(n_blocks: int, n_ranges: int, max_length: int, block_bits: int) -> int:
    """a max_blocks that is always enough: every range at a block's last byte, no block shared"""
    return min(n_blocks, n_ranges * (((max_length + (1 << block_bits) - 2) >> block_bits) + 1))


def gather_frame(d_frame, offsets, lengths, max_length: int = None, max_blocks: int = None, d_out=None,
                 info: dict = None, dictionary=None, scratch=None):
    """Many byte ranges of a device-resident frame in one call: content[offsets[r] : offsets[r] + lengths[r]] for every
    r, packed in request order into d_out (uint8, made when not given).  Every distinct covering block is decoded once,
    into the scratch, and verified.  offsets / lengths: int64 or uint64 device tensors, which the host never reads --
    max_length, a hard cap on every length, is then required -- or sequences, which are uploaded; max_length may then
    be worked out here, and a range that is longer than it or leaves the content raises ValueError here.  max_blocks:
    a cap on the distinct covering blocks, by default gather_bound(), which is always enough.  `info` and dictionary
    as for read_frame.
    Enqueues and returns (d_out, out_off int64[n + 1], range_err int32[n], blocks_decoded int32[1], status int32[1]),
    all device tensors: range r lies at d_out[out_off[r] : out_off[r + 1]] when status and range_err[r] are 0 after a
    synchronise.  A range the device finds invalid has range_err EINVAL and length 0; status ENOBUFS / ENOSPC say that
    max_blocks / d_out were too small (blocks_decoded and out_off[n] say what it takes), anything else is the frame's
    own status; a block that fails costs the ranges that touch it (their range_err) and nothing else."""
    import torch
    L = N.lib()
    if info is None:
        info = frame_info(d_frame[:HEADER_BYTES].cpu().numpy().tobytes())
    _no_version_4(info, "gather_frame")
    n, content, bits = info["n_blocks"], info["content_bytes"], info["block_bytes"].bit_length() - 1
    device = d_frame.device
    d = _dict_dev(dictionary, 1 << info["win_bits"], device) if dictionary is not None else None
    d_offsets, h_offsets = _ranges_dev(offsets, device, "offsets")
    d_lengths, h_lengths = _ranges_dev(lengths, device, "lengths")
    count = d_offsets.numel()
    if d_lengths.numel() != count:
        raise ValueError("gather_frame: as many lengths as offsets")
    if max_length is None:
        if h_lengths is None:
            raise ValueError("gather_frame: max_length is required when the lengths are a device tensor")
        max_length = max(h_lengths, default=0)
    if h_offsets is not None and h_lengths is not None:
        for o, ln in zip(h_offsets, h_lengths):
            if ln > max_length or o > content or ln > content - o:
                raise ValueError(f"gather_frame: range ({o}, {ln}) is longer than max_length or leaves the content")
    if max_blocks is None:
        max_blocks = gather_bound(n, count, max_length, bits)
    if d_out is None:
        total = sum(h_lengths) if h_lengths is not None else count * max_length
        d_out = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
    out_off = torch.zeros(count + 1, dtype=torch.int64, device=device)
    range_err = torch.zeros(max(count, 1), dtype=torch.int32, device=device)
    blocks_decoded = torch.zeros(1, dtype=torch.int32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    if scratch is None:
        scratch = _scratch_for(device, int(L.sqz_hip_frame_gather_scratch_bytes(n, count, max_blocks, bits)))
    head = (_ptr(d_frame), d_frame.numel(), n, content, bits, _ptr(d_offsets), _ptr(d_lengths), count, max_length,
            max_blocks)
    tail = (_ptr(d_out), d_out.numel(), _ptr(out_off), _ptr(range_err), _ptr(blocks_decoded), _ptr(status),
            _ptr(scratch), scratch.numel(), _stream())
    if d is not None:
        _raise(L.sqz_hip_frame_gather_dict(*head, _ptr(d), d.numel(), *tail), "sqz_hip_frame_gather_dict")
    else:
        _raise(L.sqz_hip_frame_gather(*head, *tail), "sqz_hip_frame_gather")
    return d_out, out_off, range_err[:count], blocks_decoded, status


def update_frame(d_frame, offsets, lengths, data, max_length: int = None, max_blocks: int = None, d_out=None,
                 info: dict = None, dictionary=None, parse="greedy", scratch=None):
    """Many byte ranges written into a device-resident frame in one call: the new frame, in d_out (uint8, of the
    version's bound when not given; it must not overlap d_frame), is the frame of the content with data's bytes at
    content[offsets[r] : offsets[r] + lengths[r]] for every r -- byte for byte the encoder's frame of that content with
    the same parse.  Only the distinct covering blocks are decoded, verified, patched and encoded again; every other
    stream is carried over as it lies.  data: the ranges' bytes packed in request order, bytes-like or a uint8 device
    tensor.  offsets / lengths, max_length, max_blocks, `info` and dictionary as for gather_frame (sequences are checked
    here, ValueError; device tensors go through unread, and max_length is then required).  Where ranges overlap each
    overlapped byte is one of the candidates'.
    Enqueues and returns (d_out, frame_bytes int64[1], data_off int64[n + 1], range_err int32[n], blocks_encoded
    int32[1], status int32[1]), all device tensors: d_out[:frame_bytes] is the new frame when status is 0 after a
    synchronise, and d_out is untouched otherwise.  status: the frame's own; ERANGE when the device finds a range invalid
    (range_err EINVAL there); ENOBUFS (blocks_encoded says what max_blocks takes); ENODATA when data is shorter than the
    ranges; a touched block's decode or checksum error; E2BIG when d_out is too small (frame_bytes says what it takes)."""
    import torch
    L = N.lib()
    parse = parse_code(parse)
    if info is None:
        info = frame_info(d_frame[:HEADER_BYTES].cpu().numpy().tobytes())
    _no_version_4(info, "update_frame")
    n, content, bits = info["n_blocks"], info["content_bytes"], info["block_bytes"].bit_length() - 1
    device = d_frame.device
    d = _dict_dev(dictionary, 1 << info["win_bits"], device) if dictionary is not None else None
    d_offsets, h_offsets = _ranges_dev(offsets, device, "offsets", "update_frame")
    d_lengths, h_lengths = _ranges_dev(lengths, device, "lengths", "update_frame")
    count = d_offsets.numel()
    if d_lengths.numel() != count:
        raise ValueError("update_frame: as many lengths as offsets")
    if max_length is None:
        if h_lengths is None:
            raise ValueError("update_frame: max_length is required when the lengths are a device tensor")
        max_length = max(h_lengths, default=0)
    if h_offsets is not None and h_lengths is not None:
        for o, ln in zip(h_offsets, h_lengths):
            if ln > max_length or o > content or ln > content - o:
                raise ValueError(f"update_frame: range ({o}, {ln}) is longer than max_length or leaves the content")
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8 or data.dim() != 1:
            raise ValueError("update_frame: data tensor must be one-dimensional uint8")
        d_data = data.contiguous().to(device)
    else:
        d_data = torch.frombuffer(bytearray(bytes(data) or b"\0"), dtype=torch.uint8)[:len(data)].to(device)
    if max_blocks is None:
        max_blocks = gather_bound(n, count, max_length, bits)
    if d_out is None:
        if info["version"] == 3:                             # with or without stored blocks: the larger bound
            bound = max(L.sqz_frame_bound_dict(content, bits, FRAME_DICT), L.sqz_frame_bound_dict(content, bits, FRAME_DICT | FRAME_STORED))
        elif info["version"] == 2:
            bound = L.sqz_frame_bound_ex(content, bits, FRAME_STORED)
        else:
            bound = L.sqz_frame_bound(content, bits)
        d_out = torch.empty(max(int(bound), 1), dtype=torch.uint8, device=device)
    frame_bytes = torch.zeros(1, dtype=torch.int64, device=device)
    data_off = torch.zeros(count + 1, dtype=torch.int64, device=device)
    range_err = torch.zeros(max(count, 1), dtype=torch.int32, device=device)
    blocks_encoded = torch.zeros(1, dtype=torch.int32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    if scratch is None:
        scratch = _scratch_for(device, int(L.sqz_hip_frame_update_scratch_bytes(n, count, max_blocks, bits,
                                                                                  d.numel() if d is not None else 0)))
    head = (_ptr(d_frame), d_frame.numel(), n, content, info["win_bits"], bits, _ptr(d_offsets), _ptr(d_lengths), count,
            max_length, max_blocks, _ptr(d_data) if d_data.numel() else None, d_data.numel(), _ptr(data_off), parse)
    tail = (_ptr(d_out), d_out.numel(), _ptr(frame_bytes), _ptr(range_err), _ptr(blocks_encoded), _ptr(status),
            _ptr(scratch), scratch.numel(), _stream())
    if d is not None:
        _raise(L.sqz_hip_frame_update_dict(*head, _ptr(d), d.numel(), *tail), "sqz_hip_frame_update_dict")
    else:
        _raise(L.sqz_hip_frame_update(*head, *tail), "sqz_hip_frame_update")
    return d_out, frame_bytes, data_off, range_err[:count], blocks_encoded, status


def _frame_bound_of(info: dict, content: int, bits: int) -> int:
    """a capacity that is always enough for a frame of `content` bytes at the version of `info`"""
    L = N.lib()
    if info["version"] == 3:                                 # with or without stored blocks: the larger bound
        return int(max(L.sqz_frame_bound_dict(content, bits, FRAME_DICT),
                       L.sqz_frame_bound_dict(content, bits, FRAME_DICT | FRAME_STORED)))
    if info["version"] == 2:
        return int(L.sqz_frame_bound_ex(content, bits, FRAME_STORED))
    return int(L.sqz_frame_bound(content, bits))


def append_frame(d_frame, data, d_out=None, info: dict = None, dictionary=None, parse="greedy", scratch=None):
    """More content behind a device-resident frame in one call: the new frame, in d_out (uint8, of the version's bound
    of the longer content when not given; it must not overlap d_frame), is the frame of content || data -- byte for
    byte the encoder's frame of it with the same parse.  Only a ragged last block is decoded, verified and encoded again
    with the data behind it; every other stream is carried over as it lies.  data: bytes-like or a one-dimensional
    uint8 device tensor (anything else is ValueError).  `info` and dictionary as for gather_frame.  The scratch takes
    about 11 bytes per byte of data: a long append goes in pieces, and two appends leave the frame of one.
    Enqueues and returns (d_out, frame_bytes int64[1], blocks_encoded int32[1], status int32[1]), all device tensors:
    d_out[:frame_bytes] is the new frame when status is 0 after a synchronise, and d_out is untouched otherwise.
    status: the frame's own; the last block's decode or checksum error; an encoder's errno; E2BIG when d_out is too
    small (frame_bytes says what it takes)."""
    import torch
    L = N.lib()
    parse = parse_code(parse)
    if info is None:
        info = frame_info(d_frame[:HEADER_BYTES].cpu().numpy().tobytes())
    _no_version_4(info, "append_frame")
    n, content, bits = info["n_blocks"], info["content_bytes"], info["block_bytes"].bit_length() - 1
    device = d_frame.device
    d = _dict_dev(dictionary, 1 << info["win_bits"], device) if dictionary is not None else None
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8 or data.dim() != 1:
            raise ValueError("append_frame: data tensor must be one-dimensional uint8")
        d_data = data.contiguous().to(device)
    else:
        try:
            host = bytes(memoryview(data))
        except TypeError:
            raise ValueError("append_frame: data must be bytes-like or a one-dimensional uint8 tensor") from None
        d_data = torch.frombuffer(bytearray(host or b"\0"), dtype=torch.uint8)[:len(host)].to(device)
    count = d_data.numel()
    if d_out is None:
        d_out = torch.empty(max(_frame_bound_of(info, content + count, bits), 16), dtype=torch.uint8, device=device)
    frame_bytes = torch.zeros(1, dtype=torch.int64, device=device)
    blocks_encoded = torch.zeros(1, dtype=torch.int32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    if scratch is None:
        scratch = _scratch_for(device, int(L.sqz_hip_frame_append_scratch_bytes(n, content, count, bits,
                                                                                  d.numel() if d is not None else 0)))
    head = (_ptr(d_frame), d_frame.numel(), n, content, info["win_bits"], bits, _ptr(d_data) if count else None, count,
            parse)
    tail = (_ptr(d_out), d_out.numel(), _ptr(frame_bytes), _ptr(blocks_encoded), _ptr(status), _ptr(scratch),
            scratch.numel(), _stream())
    if d is not None:
        _raise(L.sqz_hip_frame_append_dict(*head, _ptr(d), d.numel(), *tail), "sqz_hip_frame_append_dict")
    else:
        _raise(L.sqz_hip_frame_append(*head, *tail), "sqz_hip_frame_append")
    return d_out, frame_bytes, blocks_encoded, status


# ---- many frames in one call ("Batches of frames") ------------------------
def _frames_sizes(sizes, who):
    host = [int(v) for v in sizes]
    if any(v < 0 or v >> 62 for v in host):
        raise ValueError(f"{who}: sizes must be 0 .. 2^62 - 1")
    return host


def _frames_bits(win_bits, block_bits, who):
    if isinstance(block_bits, bool) or not isinstance(block_bits, int) or not 12 <= block_bits <= 24:
        raise ValueError(f"{who}: block_bits must be 12 .. 24, not {block_bits!r}")
    if win_bits is not None and (isinstance(win_bits, bool) or not isinstance(win_bits, int) or not 10 <= win_bits <= 15):
        raise ValueError(f"{who}: win_bits must be 10 .. 15, not {win_bits!r}")


_host_tables = collections.deque(maxlen=64)


def _pinned(array):
    """a numpy array's bytes in page-locked host memory, for a copy the stream makes later: the call returns before
    the copy has run, so the last tables are kept alive here rather than by the caller"""
    import numpy as np
    import torch
    table = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).pin_memory()
    _host_tables.append(table)
    return table


def _frames_shuffle(shuffle, k, who):
    """shuffle= of a batch call: None for the call as it always was (None or 0), else k element sizes out of 0, 2, 4, 8
    (an int for every frame, or a sequence with one per frame); anything else is ValueError"""
    if shuffle is None:
        return None
    if isinstance(shuffle, bool):
        raise ValueError(f"{who}: shuffle must be None, 0, 2, 4, 8 or a sequence of these, not {shuffle!r}")
    if isinstance(shuffle, int):
        if shuffle not in (0, 2, 4, 8):
            raise ValueError(f"{who}: shuffle must be 0, 2, 4 or 8, not {shuffle!r}")
        return None if shuffle == 0 else [shuffle] * k
    if isinstance(shuffle, (str, bytes, bytearray)):
        raise ValueError(f"{who}: shuffle must be None, 0, 2, 4, 8 or a sequence of these, not {shuffle!r}")
    try:
        elems = list(shuffle)
    except TypeError:
        raise ValueError(f"{who}: shuffle must be None, 0, 2, 4, 8 or a sequence of these, not {shuffle!r}") from None
    if len(elems) != k:
        raise ValueError(f"{who}: shuffle has {len(elems)} element sizes for {k} frames")
    for e in elems:
        if isinstance(e, bool) or not isinstance(e, int) or e not in (0, 2, 4, 8):
            raise ValueError(f"{who}: every element size must be 0, 2, 4 or 8, not {e!r}")
    return [int(e) for e in elems]


def frames_bound(sizes, block_bits: int = 18, store: bool = False, shuffle=None):
    """Where encode_frames puts the frames of contents of `sizes` bytes: (total, frame_at) -- frame f starts at
    frame_at[f], a multiple of 16, and has its worst-case size (frame_bound) of room; total is the size of the
    buffer.  shuffle: as for encode_frames -- a shuffled frame has 8 bytes more in front of its payload.
    Host code: no device is touched."""
    host = _frames_sizes(sizes, "frames_bound")
    _frames_bits(None, block_bits, "frames_bound")
    k = len(host)
    elems = _frames_shuffle(shuffle, k, "frames_bound")
    arr = (C.c_uint64 * max(k, 1))(*host)
    at = (C.c_uint64 * (k + 1))()
    if elems is not None:
        el = (C.c_uint32 * max(k, 1))(*elems)
        total = int(N.lib().sqz_hip_frames_bound_shuf(arr, el, k, block_bits, _flags(store), at))
    else:
        total = int(N.lib().sqz_hip_frames_bound(arr, k, block_bits, _flags(store), at))
    if total == 0 and k > 0:
        raise ValueError("frames_bound: the sizes add up to more than a batch holds")
    return total, [int(v) for v in at[:k]]


def encode_frames(d_in, sizes, win_bits: int = 15, block_bits: int = 18, store: bool = False, parse: str = "greedy",
                  d_out=None, scratch=None, shuffle=None):
    """Many frames in one call: the contents lie back to back in d_in (uint8), sizes[f] bytes each, and frame f is
    written at d_frames[frame_at[f]:] -- byte for byte the frame FrameEncoder writes for that content alone with the
    same arguments (versions 1 and 2).  The launches do not depend on the number of frames.
    shuffle: None or 0 is the call as it always was.  2, 4 or 8 shuffles every frame with that element size; a sequence
    of len(sizes) values out of 0, 2, 4, 8 gives every frame its own (0: not shuffled) -- frame f is then byte for byte
    FrameEncoder(..., shuffle=shuffle[f])'s, version 4 where it is shuffled; one more launch shuffles the whole batch.
    Enqueues and returns (d_frames, frame_at, d_frame_bytes int64[k], d_err int32[total blocks], d_status int32[k]):
    frame_at is frames_bound()'s host list, everything else device tensors to read after a synchronise.  Frame f is
    d_frames[frame_at[f] : frame_at[f] + d_frame_bytes[f]] when d_status[f] is 0; a frame with a failed block has
    that block's errno there and is not written, which costs its neighbours nothing.  The bytes between two frames are
    not touched.  d_out: a uint8 tensor of at least frames_bound()'s total, made when not given."""
    import numpy as np
    import torch
    code = parse_code(parse)
    host = _frames_sizes(sizes, "encode_frames")
    _frames_bits(win_bits, block_bits, "encode_frames")
    k = len(host)
    elems = _frames_shuffle(shuffle, k, "encode_frames")
    L = N.lib()
    total, frame_at = frames_bound(host, block_bits, store, elems)
    if d_in.dtype != torch.uint8 or d_in.dim() != 1 or d_in.numel() < sum(host):
        raise ValueError("encode_frames: d_in must be a one-dimensional uint8 tensor that holds all the contents")
    device = d_in.device
    if d_out is None:
        d_out = torch.empty(max(total, 16), dtype=torch.uint8, device=device)
    elif d_out.dtype != torch.uint8 or d_out.numel() < total:
        raise ValueError("encode_frames: d_out must be a uint8 tensor of at least frames_bound()'s total")
    blocks = sum((v + (1 << block_bits) - 1) >> block_bits for v in host)
    frame_bytes = torch.zeros(max(k, 1), dtype=torch.int64, device=device)
    status = torch.zeros(max(k, 1), dtype=torch.int32, device=device)
    err = torch.zeros(max(blocks, 1), dtype=torch.int32, device=device)
    table = _pinned(np.asarray(host, np.uint64)) if k > 0 else None
    if elems is not None:
        el = _pinned(np.asarray(elems, np.uint32)) if k > 0 else None
        if scratch is None:
            need = int(L.sqz_hip_frames_encode_scratch_bytes_shuf(_ptr(table), _ptr(el), k, block_bits, _flags(store)))
            scratch = _scratch_for(device, max(need, 16))
        _raise(L.sqz_hip_frames_encode_shuf(_ptr(d_in), _ptr(table), _ptr(el), k, win_bits, block_bits, _flags(store),
                                            code, _ptr(d_out), d_out.numel(), _ptr(frame_bytes), _ptr(status), _ptr(err),
                                            _ptr(scratch), scratch.numel(), _stream()), "sqz_hip_frames_encode_shuf")
        return d_out, frame_at, frame_bytes[:k], err[:blocks], status[:k]
    if scratch is None:
        need = int(L.sqz_hip_frames_encode_scratch_bytes(_ptr(table), k, block_bits, _flags(store)))
        scratch = _scratch_for(device, max(need, 16))
    _raise(L.sqz_hip_frames_encode(_ptr(d_in), _ptr(table), k, win_bits, block_bits, _flags(store), code, _ptr(d_out),
                                   d_out.numel(), _ptr(frame_bytes), _ptr(status), _ptr(err), _ptr(scratch),
                                   scratch.numel(), _stream()), "sqz_hip_frames_encode")
    return d_out, frame_at, frame_bytes[:k], err[:blocks], status[:k]


def _headers_dev(d_frames, frame_at):
    """the 32-byte headers of the frames at frame_at, read back from the device in one copy"""
    import torch
    at = torch.tensor(frame_at, dtype=torch.int64, device=d_frames.device)
    idx = at[:, None] + torch.arange(HEADER_BYTES, device=d_frames.device)[None, :]
    raw = d_frames[idx.reshape(-1)].cpu().numpy().tobytes()
    return [raw[HEADER_BYTES * f:HEADER_BYTES * (f + 1)] for f in range(len(frame_at))]


def _info_or_nothing(header: bytes):
    """frame_info() of a header, or the figures of an empty frame for a header that does not parse: the device
    refuses such a frame by the same checks, and alone"""
    try:
        return frame_info(header)
    except SqzError:
        return {"n_blocks": 0, "content_bytes": 0}


def _records_dev(d_frames, frame_at, infos):
    """the element sizes of the version-4 frames among `infos`, read from the 8-byte records behind their indexes in
    one gathered copy (0 for every other frame, and for a record out of reach or with no element size in it: the
    device refuses such a frame, and alone)"""
    import torch
    elems = [0] * len(infos)
    where = [(f, frame_at[f] + HEADER_BYTES + 8 * int(i["n_blocks"])) for f, i in enumerate(infos)
             if i.get("version") == 4]
    where = [(f, a) for f, a in where if a + 8 <= d_frames.numel()]
    if where:
        at = torch.tensor([a for _, a in where], dtype=torch.int64, device=d_frames.device)
        idx = at[:, None] + torch.arange(8, device=d_frames.device)[None, :]
        raw = d_frames[idx.reshape(-1)].cpu().numpy().tobytes()
        for j, (f, _) in enumerate(where):
            e = int.from_bytes(raw[8 * j:8 * j + 4], "little")
            elems[f] = e if e in (2, 4, 8) else 0
    return elems


def decode_frames(d_frames, frame_at, infos=None, d_out=None, out_at=None, scratch=None, shuffled: bool = False):
    """Many device-resident frames in one call: frame f lies at d_frames[frame_at[f]:] (frame_at: ascending multiples
    of 16; a frame reaches at most to the next one, the last to the end of the tensor), any mix of versions 1 and 2,
    each with its own win_bits and block_bits.  infos: a list of frame_info() dicts of the headers; without it the
    headers are read back from the device in one copy.  Frame f's content goes to d_out[out_at[f]:]; out_at defaults
    to the contents packed back to back (gaps are allowed and stay untouched, but cost scratch), d_out is made when
    not given.  The launches do not depend on the number of frames.
    Enqueues and returns (d_out, out_at, d_err int32[total blocks], d_status int32[k]); frame f's blocks are
    d_err[sum(n_blocks[:f]):].  A frame that is refused (a header or index that does not hold; version 3 or 4: EINVAL)
    has its status in d_status[f] and in all its d_err, and nothing of its output is written; a block whose checksum
    does not hold is EILSEQ in d_err.  Either costs the other frames nothing.
    shuffled=True takes versions 1, 2 and 4 in any mix (version 3 stays EINVAL): a version-4 frame is decoded by
    infos[f]["elem_bytes"] (frame_info() of header, index AND record); without infos the records of the version-4
    frames are read from the device in one more gathered copy.  One more launch shuffles the whole batch back."""
    import numpy as np
    import torch
    frame_at = [int(v) for v in frame_at]
    k = len(frame_at)
    if any(v < 0 or v % 16 != 0 for v in frame_at):
        raise ValueError("decode_frames: every frame_at must be a multiple of 16")
    if infos is not None and len(infos) != k:
        raise ValueError("decode_frames: as many infos as frame_at")
    if out_at is not None and len(out_at) != k:
        raise ValueError("decode_frames: as many out_at as frame_at")
    if d_frames.dtype != torch.uint8 or d_frames.dim() != 1:
        raise ValueError("decode_frames: d_frames must be a one-dimensional uint8 tensor")
    if any(b <= a for a, b in zip(frame_at, frame_at[1:])) or (k > 0 and frame_at[-1] >= max(d_frames.numel(), 1)):
        raise ValueError("decode_frames: frame_at must be ascending and inside d_frames")
    L = N.lib()
    device = d_frames.device
    elems = [0] * k
    if infos is None:
        infos = [_info_or_nothing(h) for h in _headers_dev(d_frames, frame_at)] if k > 0 else []
        if shuffled:
            elems = _records_dev(d_frames, frame_at, infos)
    elif shuffled:
        elems = [int(i.get("elem_bytes") or 0) if i.get("version") == 4 else 0 for i in infos]
        elems = [e if e in (2, 4, 8) else 0 for e in elems]
    sizes = [int(i["content_bytes"]) for i in infos]
    counts = [int(i["n_blocks"]) for i in infos]
    if out_at is None:
        out_at = [sum(sizes[:f]) for f in range(k)]
    out_at = [int(v) for v in out_at]
    end = max([o + s for o, s in zip(out_at, sizes)], default=0)
    if d_out is None:
        d_out = torch.empty(max(end, 1), dtype=torch.uint8, device=device)
    elif d_out.dtype != torch.uint8 or d_out.numel() < end:
        raise ValueError("decode_frames: d_out must be a uint8 tensor that holds every output")
    ends = frame_at[1:] + [d_frames.numel()]
    items = np.zeros(max(k, 1), np.dtype([("frame_at", "<u8"), ("avail", "<u8"), ("content_bytes", "<u8"),
                                          ("out_at", "<u8"), ("n_blocks", "<u4"), ("zero", "<u4")]))
    for f in range(k):
        items[f] = (frame_at[f], ends[f] - frame_at[f], sizes[f], out_at[f], counts[f], elems[f])
    table = _pinned(items) if k > 0 else None
    blocks = sum(counts)
    err = torch.zeros(max(blocks, 1), dtype=torch.int32, device=device)
    status = torch.zeros(max(k, 1), dtype=torch.int32, device=device)
    if k > 0 and shuffled:
        if scratch is None:
            need = int(L.sqz_hip_frames_decode_scratch_bytes_shuf(_ptr(table), k))
            if need == 0:
                raise ValueError("decode_frames: frames or outputs that are not ascending and disjoint")
            scratch = _scratch_for(device, need)
        _raise(L.sqz_hip_frames_decode_shuf(_ptr(d_frames), _ptr(table), k, _ptr(d_out), _ptr(err), _ptr(status),
                                            _ptr(scratch), scratch.numel(), _stream()), "sqz_hip_frames_decode_shuf")
    elif k > 0:
        if scratch is None:
            need = int(L.sqz_hip_frames_decode_scratch_bytes(_ptr(table), k))
            if need == 0:
                raise ValueError("decode_frames: frames or outputs that are not ascending and disjoint")
            scratch = _scratch_for(device, need)
        _raise(L.sqz_hip_frames_decode(_ptr(d_frames), _ptr(table), k, _ptr(d_out), _ptr(err), _ptr(status),
                                       _ptr(scratch), scratch.numel(), _stream()), "sqz_hip_frames_decode")
    return d_out, out_at, err[:blocks], status[:k]


def compress_frames(datas, win_bits: int = 15, block_bits: int = 18, store: bool = False,
                    parse: str = "greedy", shuffle=None) -> list:
    """compress_frame() of every item of `datas` (versions 1 and 2) in one device call: one upload, one synchronise,
    one download.  Raises SqzError naming the first frame that failed.
    shuffle: as for encode_frames -- compress_frame(d, ..., shuffle=e) for every item, or for item f with shuffle[f]."""
    import torch
    parse_code(parse)                                        # argument errors before anything is uploaded
    _frames_bits(win_bits, block_bits, "compress_frames")
    datas = [bytes(d) for d in datas]
    elems = _frames_shuffle(shuffle, len(datas), "compress_frames")
    if not datas:
        return []
    blob = b"".join(datas)
    d_in = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8)[:len(blob)].to("cuda")
    d_frames, frame_at, frame_bytes, _, status = encode_frames(d_in, [len(d) for d in datas], win_bits, block_bits,
                                                               store, parse, shuffle=elems)
    torch.cuda.synchronize()
    sizes, states = frame_bytes.cpu().tolist(), status.cpu().tolist()
    for f, st in enumerate(states):
        if st != 0:
            raise SqzError(st, f"compress_frames: frame {f}: {errno.errorcode.get(st, st)}")
    host = d_frames.cpu().numpy()
    return [host[a:a + n].tobytes() for a, n in zip(frame_at, sizes)]


def decompress_frames(frames, return_errors: bool = False, shuffled: bool = False):
    """decompress_frame() of every item of `frames` (versions 1 and 2, any mix of parameters) in one device call: one
    upload, one synchronise, one download.  Raises SqzError naming the first frame that did not hold -- its status, or
    its first failed block -- unless return_errors is set: then (contents, errors) with errors[f] = (status,
    block_errors); good frames and good blocks are delivered, a refused frame is b"".
    shuffled=True takes version 4 as well (decode_frames); the element sizes are read from the frames' records."""
    import numpy as np
    import torch
    frames = [bytes(f) for f in frames]
    if not frames:
        return ([], []) if return_errors else []
    infos = [_info_or_nothing(f[:HEADER_BYTES]) if len(f) >= HEADER_BYTES else {"n_blocks": 0, "content_bytes": 0}
             for f in frames]
    frame_at, at = [], 0
    for f in frames:
        frame_at.append(at)
        at += (max(len(f), HEADER_BYTES) + 15) & ~15
    image = np.zeros(at + 16, np.uint8)
    for a, f in zip(frame_at, frames):
        image[a:a + len(f)] = np.frombuffer(f, np.uint8)
    d_frames = torch.from_numpy(image)[:at].to("cuda")
    if shuffled:                                             # the records are at hand: no copy back from the device
        for j, (f, info) in enumerate(zip(frames, infos)):
            at = HEADER_BYTES + 8 * info["n_blocks"]
            if info.get("version") == 4 and len(f) >= at + 8:
                infos[j] = dict(info, elem_bytes=int.from_bytes(f[at:at + 4], "little"))
    d_out, out_at, err, status = decode_frames(d_frames, frame_at, infos, shuffled=shuffled)
    torch.cuda.synchronize()
    host, errs, states = d_out.cpu().numpy(), err.cpu().tolist(), status.cpu().tolist()
    contents, errors, b0 = [], [], 0
    for f, info in enumerate(infos):
        n = info["n_blocks"]
        block_errors = errs[b0:b0 + n]
        b0 += n
        st = states[f]
        if not return_errors and (st != 0 or any(block_errors)):
            first = st if st != 0 else next(e for e in block_errors if e != 0)
            e = SqzError(first, f"decompress_frames: frame {f}: {errno.errorcode.get(first, first)}")
            e.frame, e.block_errors = f, block_errors
            raise e
        contents.append(b"" if st != 0 else host[out_at[f]:out_at[f] + info["content_bytes"]].tobytes())
        errors.append((st, block_errors))
    return (contents, errors) if return_errors else contents


def _append_file(frame: bytes, data: bytes, dictionary, parse: str) -> bytes:
    """the file tool's `a`: FRAME and IN through append_frame, the new frame as bytes (SqzError on a status)"""
    _no_version_4(frame_info(frame[:HEADER_BYTES]), "append")       # before anything native, torch included, runs
    import torch
    d_frame = torch.frombuffer(bytearray(frame) + bytearray(16), dtype=torch.uint8)[:len(frame)].to("cuda")
    d_out, frame_bytes, _, status = append_frame(d_frame, data, info=frame_info(frame), dictionary=dictionary,
                                                 parse=parse)
    torch.cuda.synchronize()
    _raise(int(status.item()), "append_frame (status)")
    return d_out[:int(frame_bytes.item())].cpu().numpy().tobytes()


# ---- file tool ----------------------------------------------------------------------------------
def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m sqz_amd.frame", description="SQZF frames of files")
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("c", help="compress IN to OUT")
    c.add_argument("src")
    c.add_argument("dst")
    c.add_argument("--win-bits", type=int, default=15)
    c.add_argument("--block-bits", type=int, default=18)
    c.add_argument("--store", action="store_true", help="version 2: store a block whose stream is not smaller")
    c.add_argument("--lazy", action="store_true", help="lazy parse: smaller streams, same format (not the reference's bytes)")
    c.add_argument("--dict", dest="dictionary", metavar="FILE",
                   help="version 3: every block may reach back into FILE's bytes (1 .. window - 1 of them)")
    c.add_argument("--shuffle", type=int, default=0, metavar="N",
                   help="version 4: byte-shuffle every block as elements of N = 2, 4 or 8 bytes (not with --dict)")
    d = sub.add_parser("d", help="decompress IN to OUT")
    d.add_argument("src")
    d.add_argument("dst")
    d.add_argument("--dict", dest="dictionary", metavar="FILE", help="the dictionary a version-3 frame was written with")
    p = sub.add_parser("a", help="append IN's bytes to FRAME, write OUT")
    p.add_argument("frame")
    p.add_argument("src")
    p.add_argument("dst")
    p.add_argument("--lazy", action="store_true", help="lazy parse for the blocks that are encoded")
    p.add_argument("--dict", dest="dictionary", metavar="FILE", help="the dictionary a version-3 frame was written with")
    i = sub.add_parser("info", help="describe IN")
    i.add_argument("src")
    k = sub.add_parser("blocks", help="one line per block of IN")
    k.add_argument("src")
    a = ap.parse_args(argv)
    with open(a.src, "rb") as fh:
        blob = fh.read()
    dct = None
    if getattr(a, "dictionary", None):
        with open(a.dictionary, "rb") as fh:
            dct = fh.read()
    try:
        if a.cmd == "c":
            parse = "lazy" if a.lazy else "greedy"
            if a.shuffle != 0:
                out = compress_frame(blob, a.win_bits, a.block_bits, a.store, parse, dictionary=dct, shuffle=a.shuffle)
            elif dct is None:
                out = compress_frame(blob, a.win_bits, a.block_bits, a.store, parse)
            else:
                out = compress_frame(blob, a.win_bits, a.block_bits, a.store, parse, dictionary=dct)
        elif a.cmd == "a":
            with open(a.frame, "rb") as fh:
                out = _append_file(fh.read(), blob, dct, "lazy" if a.lazy else "greedy")
        elif a.cmd == "d":
            out = decompress_frame(blob) if dct is None else decompress_frame(blob, dictionary=dct)
        elif a.cmd == "blocks":
            for b, blk in enumerate(frame_blocks(blob)):
                print(f"{b}: " + " ".join(f"{key}={v}" for key, v in blk.items()))
            return 0
        else:
            for k, v in frame_info(blob).items():
                print(f"{k}: {v}")
            return 0
    except (SqzError, ValueError) as e:
        print(f"sqz_amd.frame: {e}", flush=True)
        return 1
    with open(a.dst, "wb") as fh:
        fh.write(out)
    print(f"{a.src}: {len(blob)} -> {len(out)} bytes")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
