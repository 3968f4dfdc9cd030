"""PNG files with the standard library only (zlib, struct): what image/png.Encode gives gsdfaux.RenderPNGFile, as plain 8-bit RGBA."""
import struct
import zlib

import numpy as np


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)


def write_png(path, rgba):
    """8-bit RGBA PNG of an (h, w, 4) uint8 array, rows from the top (filter 0 on every row)."""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    assert rgba.shape == (h, w, 4), rgba.shape
    raw = np.zeros((h, 1 + 4 * w), np.uint8)
    raw[:, 1:] = rgba.reshape(h, 4 * w)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _chunk(b"IEND", b""))


def read_png(path):
    """The pixels of a PNG written by write_png (8-bit RGBA, no interlace, filter 0): (h, w, 4) uint8."""
    data = open(path, "rb").read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG file")
    off, idat, w, h = 8, b"", None, None
    while off < len(data):
        n, = struct.unpack(">I", data[off:off + 4])
        kind, body = data[off + 4:off + 8], data[off + 8:off + 8 + n]
        if zlib.crc32(kind + body) & 0xffffffff != struct.unpack(">I", data[off + 8 + n:off + 12 + n])[0]:
            raise ValueError("bad chunk CRC")
        if kind == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body[:13])
            if depth != 8 or ctype != 6 or interlace != 0:
                raise ValueError("only 8-bit RGBA, non-interlaced PNGs are read")
        elif kind == b"IDAT":
            idat += body
        off += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)
    if (raw[:, 0] != 0).any():
        raise ValueError("only filter 0 rows are read")
    return raw[:, 1:].reshape(h, w, 4).copy()
