"""Host-side PNG writer for the visual mode (main.py:638-646 saves its pictures through matplotlib): 8-bit RGBA, one IDAT
chunk, filter type 0 on every row -- the PNG specification's layout restated with zlib and struct, no imaging library."""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_rgba(path, array: np.ndarray) -> None:
    """Write `array` (numpy uint8 [H,W,4]: r, g, b, a) as an 8-bit RGBA PNG."""
    if not isinstance(array, np.ndarray) or array.dtype != np.uint8 or array.ndim != 3 or array.shape[2] != 4 or 0 in array.shape:
        raise ValueError(f"png.write_rgba: a uint8 [H,W,4] numpy array is needed (got {getattr(array, 'dtype', type(array))}, "
                         f"shape {getattr(array, 'shape', None)})")
    h, w = array.shape[:2]
    rows = np.zeros((h, 1 + 4 * w), dtype=np.uint8)              # column 0: the filter type byte of each row (0 = None)
    rows[:, 1:] = array.reshape(h, 4 * w)
    with open(os.fspath(path), "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b""))
