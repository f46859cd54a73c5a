"""A minimal PNG writer (stdlib zlib + struct, filter type 0 on every row): 16-bit gray for depth images in the TUM RGB-D
layout, 8-bit gray and 8-bit RGB for colour.  Reading goes through the C++ reader (badslam_amd.direct_ba.read_png)."""
import struct
import zlib

import numpy as np

_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(image, compression=6):
    """(h, w) uint16 -> 16-bit gray; (h, w) uint8 -> 8-bit gray; (h, w, 3) uint8 -> 8-bit RGB.  Returns the file's bytes."""
    a = np.asarray(image)
    if a.ndim == 2 and a.dtype == np.uint16:
        bit_depth, color_type, rows = 16, 0, a.astype(">u2").view(np.uint8).reshape(a.shape[0], -1)
    elif a.ndim == 2 and a.dtype == np.uint8:
        bit_depth, color_type, rows = 8, 0, a
    elif a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8:
        bit_depth, color_type, rows = 8, 2, a.reshape(a.shape[0], -1)
    else:
        raise ValueError(f"cannot write an array of shape {a.shape} and type {a.dtype} as PNG")
    h, w = a.shape[:2]
    if h < 1 or w < 1:
        raise ValueError("a PNG needs at least one pixel")
    raw = np.zeros((h, 1 + rows.shape[1]), np.uint8)   # column 0: filter type 0 (none)
    raw[:, 1:] = rows
    header = struct.pack(">IIBBBBB", w, h, bit_depth, color_type, 0, 0, 0)
    return _SIGNATURE + _chunk(b"IHDR", header) + _chunk(b"IDAT", zlib.compress(raw.tobytes(), compression)) + _chunk(b"IEND", b"")


def write_png(path, image, compression=6):
    with open(path, "wb") as f:
        f.write(encode_png(image, compression))
