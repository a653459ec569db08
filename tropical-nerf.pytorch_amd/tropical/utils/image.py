"""8-bit RGBA PNG files with the standard library only (zlib, struct): the
files `tropical.stanford.visualize` writes, and a reader for exactly that
subset (colour type 6, bit depth 8, no interlace, filter 0 on every row)."""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np

_SIG = b"\x89PNG\r\n\x1a\n"


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path: str, rgba) -> None:
    """rgba: uint8 [H, W, 4] (numpy array or tensor on any device)."""
    if hasattr(rgba, "detach"):
        rgba = rgba.detach().cpu().numpy()
    a = np.ascontiguousarray(rgba)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: uint8 [H, W, 4] with H, W >= 1 expected, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 4 * w), dtype=np.uint8)  # filter byte 0, then the row
    rows[:, 1:] = a.reshape(h, 4 * w)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "wb") as f:
        f.write(_SIG)
        f.write(_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)))
        f.write(_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        f.write(_chunk(b"IEND", b""))


def read_png(path: str) -> np.ndarray:
    """uint8 [H, W, 4] of a file write_png wrote; anything else is refused."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _SIG:
        raise ValueError(f"{path}: not a PNG file")
    pos, head, idat = 8, None, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if crc != zlib.crc32(kind + body) & 0xFFFFFFFF:
            raise ValueError(f"{path}: bad CRC in chunk {kind!r}")
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        pos += 12 + n
    if head is None or head[2:] != (8, 6, 0, 0, 0):
        raise ValueError(f"{path}: only 8-bit RGBA without interlace is read (IHDR {head})")
    w, h = head[:2]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if raw.size != h * (1 + 4 * w):
        raise ValueError(f"{path}: {raw.size} bytes of image data, {h * (1 + 4 * w)} expected")
    rows = raw.reshape(h, 1 + 4 * w)
    if rows[:, 0].any():
        raise ValueError(f"{path}: only filter 0 is read")
    return rows[:, 1:].reshape(h, w, 4).copy()
