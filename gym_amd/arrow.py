"""Pendulum-v1's torque arrow: the image its frame blits (pendulum.py:228-244, assets/clockwise.png).

The engine does not carry the reference's asset; the caller passes it (`arrow_image=`), as an array or as a path to the PNG.  The PNG is
read by a small decoder written from the PNG specification (W3C, 2nd edition: chunks, zlib stream, scanline filters 0-4), with the
standard library's zlib only, for what such an asset is: 8 bits per channel, not interlaced, RGB or RGBA.  Anything else is refused with
a ValueError that says to decode it elsewhere and pass the array.
"""
from __future__ import annotations

import importlib.util
import os
import struct
import zlib
from typing import Optional

import numpy as np

PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_SIDE = 1024
ASSET = os.path.join("envs", "classic_control", "assets", "clockwise.png")
PASS_AN_ARRAY = "decode it with an image library and pass arrow_image= a uint8 (H, W, 4) RGBA array instead"


def _paeth(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def decode_png(data: bytes) -> np.ndarray:
    """uint8 (H, W, 4) straight RGBA of an 8-bit, non-interlaced PNG of colour type 2 (RGB: alpha 255) or 6 (RGBA)."""
    if data[:8] != PNG_SIGNATURE:
        raise ValueError(f"not a PNG file (bad signature): {PASS_AN_ARRAY}")
    pos, header, idat = 8, None, []
    while pos + 8 <= len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + length]
        if len(body) != length or pos + 12 + length > len(data):
            raise ValueError(f"truncated PNG chunk {kind!r}: {PASS_AN_ARRAY}")
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        if zlib.crc32(kind + body) & 0xFFFFFFFF != crc:
            raise ValueError(f"PNG chunk {kind!r} fails its CRC: {PASS_AN_ARRAY}")
        pos += 12 + length
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if header is None or not idat:
        raise ValueError(f"PNG without IHDR or IDAT: {PASS_AN_ARRAY}")
    width, height, depth, ctype, compression, filt, interlace = header
    if depth != 8 or ctype not in (2, 6) or compression != 0 or filt != 0 or interlace != 0:
        raise ValueError(f"unsupported PNG (bit depth {depth}, colour type {ctype}, interlace {interlace}); this decoder reads 8-bit, "
                         f"non-interlaced RGB / RGBA only: {PASS_AN_ARRAY}")
    if width < 1 or height < 1:
        raise ValueError(f"empty PNG: {PASS_AN_ARRAY}")
    bpp = 3 if ctype == 2 else 4
    stride = width * bpp
    raw = zlib.decompress(b"".join(idat))
    if len(raw) < height * (stride + 1):
        raise ValueError(f"PNG image data too short: {PASS_AN_ARRAY}")
    rows = np.frombuffer(raw, np.uint8, height * (stride + 1)).reshape(height, stride + 1)
    out = np.zeros((height, stride), np.int32)
    prev = np.zeros(stride, np.int32)
    for y in range(height):
        f, line = rows[y, 0], rows[y, 1:].astype(np.int32)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        elif f in (1, 3, 4):
            # the left neighbour depends on the row's own output: one pixel at a time, bpp bytes at once
            cur = np.zeros(stride, np.int32)
            zero = np.zeros(bpp, np.int32)
            for x in range(0, stride, bpp):
                left = cur[x - bpp:x] if x else zero
                up = prev[x:x + bpp]
                upleft = prev[x - bpp:x] if x else zero
                pred = left if f == 1 else (left + up) // 2 if f == 3 else _paeth(left, up, upleft)
                cur[x:x + bpp] = (line[x:x + bpp] + pred) & 255
        else:
            raise ValueError(f"PNG scanline filter {int(f)} is not one of 0-4: {PASS_AN_ARRAY}")
        out[y] = cur
        prev = cur
    img = out.astype(np.uint8).reshape(height, width, bpp)
    if bpp == 3:
        img = np.concatenate([img, np.full((height, width, 1), 255, np.uint8)], axis=2)
    return np.ascontiguousarray(img)


def pendulum_arrow_image(path: Optional[str] = None) -> np.ndarray:
    """The arrow Pendulum-v1's frame blits, uint8 (H, W, 4) straight RGBA (329 x 312 for the reference's asset).  `path`: a PNG file;
    None looks for envs/classic_control/assets/clockwise.png inside an installed `gym` package (found with importlib.util.find_spec,
    gym is not imported)."""
    if path is None:
        spec = importlib.util.find_spec("gym")
        roots = list(spec.submodule_search_locations or []) if spec is not None else []
        found = [os.path.join(r, ASSET) for r in roots if os.path.isfile(os.path.join(r, ASSET))]
        if not found:
            raise FileNotFoundError("Pendulum-v1's arrow image (gym/envs/classic_control/assets/clockwise.png) was not found: no installed "
                                    "gym package carries it.  Pass pendulum_arrow_image(path) the PNG's path, or arrow_image= a uint8 "
                                    "(H, W, 4) RGBA array")
        path = found[0]
    with open(os.fspath(path), "rb") as f:
        return decode_png(f.read())


def as_arrow_image(value) -> np.ndarray:
    """`arrow_image=` as the engine takes it: a path (str / os.PathLike) to a PNG, or an array; uint8 (H, W, 4), 1 <= H, W <= 1024,
    C-contiguous.  TypeError / ValueError otherwise (before any device work)."""
    if isinstance(value, (str, os.PathLike)):
        value = pendulum_arrow_image(value)
    if not isinstance(value, np.ndarray):
        raise TypeError(f"arrow_image must be a uint8 (H, W, 4) RGBA array or a path to a PNG, got {type(value).__name__}")
    if value.dtype != np.uint8 or value.ndim != 3 or value.shape[2] != 4:
        raise ValueError(f"arrow_image must be uint8 (H, W, 4) straight RGBA, got {value.dtype} {value.shape}")
    if not (1 <= value.shape[0] <= MAX_SIDE and 1 <= value.shape[1] <= MAX_SIDE):
        raise ValueError(f"arrow_image must be 1 .. {MAX_SIDE} pixels high and wide, got {value.shape[0]} x {value.shape[1]}")
    return np.ascontiguousarray(value)
