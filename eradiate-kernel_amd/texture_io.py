"""Bitmap files of the `bitmap` texture: Portable Float Map only.

Follows the reference's Bitmap::read_pfm (src/libcore/bitmap.cpp:2151-2204): the header is "PF" (rgb) or "Pf" (one channel) and three
whitespace-separated tokens -- width, height, scale -- each followed by ONE whitespace character; the sign of the scale gives the byte
order of the floats (<= 0: little endian), its magnitude multiplies them; the file stores the bottom row first and the reader flips it
(vflip), so row 0 of the result is the image's top row.  A PFM holds linear values: no gamma is undone (m_srgb_gamma = false).
"""
import numpy as np


def read_pfm(path):
    """-> float32 array (height, width) or (height, width, 3), top row first."""
    with open(path, "rb") as fh:
        blob = fh.read()
    if len(blob) < 3 or blob[0:1] != b"P" or blob[1:2] not in (b"F", b"f"):
        raise RuntimeError("read_pfm(): Invalid header!")
    channels = 3 if blob[1:2] == b"F" else 1
    pos, tokens = 2, []
    try:
        for _ in range(3):                                       # Stream::read_token: skip whitespace, read up to the next whitespace
            while blob[pos:pos + 1].isspace():
                pos += 1
            end = pos
            while end < len(blob) and not blob[end:end + 1].isspace():
                end += 1
            tokens.append(blob[pos:end].decode("ascii"))
            pos = end
        width, height, scale = int(tokens[0]), int(tokens[1]), float(tokens[2])
    except (ValueError, UnicodeDecodeError):
        raise RuntimeError("Could not parse PFM header!")
    pos += 1                                                     # the one whitespace character behind the scale
    count = width * height * channels
    if width <= 0 or height <= 0 or len(blob) - pos < 4 * count:
        raise RuntimeError("read_pfm(): \"%s\" holds fewer than %d x %d x %d floats" % (path, width, height, channels))
    data = np.frombuffer(blob, dtype="<f4" if scale <= 0.0 else ">f4", count=count, offset=pos).astype(np.float32)
    if abs(scale) != 1.0:
        data = data * np.float32(abs(scale))
    data = data.reshape((height, width, 3) if channels == 3 else (height, width))
    return np.ascontiguousarray(data[::-1])
