"""Host statement of the engine's pixel observations (include/mxv_render.h mxv_pixels*): frame -> gray -> area resize.

Not a test module: tests/test_pixels_host.py (CPU) and tests/test_gpu_pixels.py (device) import it.  Nothing under gym_amd/ does.

The input is a frame as tests/render_host.py draws it (uint8 [H, W, 3], row 0 at the top); the output is uint8 [h, w] (gray) or
[h, w, 3] (RGB), 1 <= h <= H, 1 <= w <= W.  Integer arithmetic only, so that the device equals it bit for bit:
  * gray, applied first (the reference's wrapper order): Y = (4899 R + 9617 G + 1868 B + 8192) >> 14 per source pixel, OpenCV's
    documented fixed-point BT.601 weights for 8-bit RGB2GRAY (not checked against cv2 here);
  * area resize: output pixel (i, j) is (sum + n // 2) // n over the n source pixels of rows [floor(i H / h), ceil((i + 1) H / h)) and
    columns [floor(j W / w), ceil((j + 1) W / w)), per channel: torch.nn.functional.adaptive_avg_pool2d's windows, so
    floor(adaptive_avg_pool2d(frame.double()) + 0.5) is an independent statement of the same numbers.  At a non-integer ratio adjacent
    windows share a row or column; this is NOT OpenCV's INTER_AREA there (which weights the shared pixel fractionally).
"""
from __future__ import annotations

import numpy as np

GRAY_WEIGHTS = (4899, 9617, 1868)   # sum 2^14


def gray(frame: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] -> uint8 [...]."""
    f = frame.astype(np.int64)
    r, g, b = GRAY_WEIGHTS
    return ((r * f[..., 0] + g * f[..., 1] + b * f[..., 2] + 8192) >> 14).astype(np.uint8)


def windows(src: int, dst: int):
    """[(lo, hi)] of the dst output positions along one axis of length src."""
    return [((i * src) // dst, -((-(i + 1) * src) // dst)) for i in range(dst)]


def area_resize(img: np.ndarray, h: int, w: int) -> np.ndarray:
    """uint8 [H, W] or [H, W, C] -> [h, w] or [h, w, C] by the rounded integer mean over each output pixel's window."""
    H, W = img.shape[:2]
    if not (1 <= h <= H and 1 <= w <= W):
        raise ValueError(f"target {h} x {w} outside [1, {H}] x [1, {W}]")
    # summed-area table: sums of any window in four lookups (at most 255 H W < 2^31: int32 is exact)
    sat = np.zeros((H + 1, W + 1) + img.shape[2:], np.int32)
    np.cumsum(img, axis=0, dtype=np.int32, out=sat[1:, 1:])
    np.cumsum(sat[1:, 1:], axis=1, out=sat[1:, 1:])
    rows, cols = np.array(windows(H, h)), np.array(windows(W, w))
    r0, r1 = rows[:, 0][:, None], rows[:, 1][:, None]
    c0, c1 = cols[:, 0][None, :], cols[:, 1][None, :]
    s = sat[r1, c1].astype(np.int64) - sat[r0, c1] - sat[r1, c0] + sat[r0, c0]
    n = (r1 - r0) * (c1 - c0)
    if s.ndim == 3:
        n = n[..., None]
    return ((s + n // 2) // n).astype(np.uint8)


def reduce(frame: np.ndarray, h: int, w: int, grayscale: bool = True) -> np.ndarray:
    """The pixel observation of one frame (uint8 [H, W, 3]) or of a batch (uint8 [k, H, W, 3])."""
    frame = np.asarray(frame)
    if frame.ndim == 4:
        return np.stack([reduce(f, h, w, grayscale) for f in frame]) if len(frame) else \
            np.zeros((0, h, w) + (() if grayscale else (3,)), np.uint8)
    return area_resize(gray(frame) if grayscale else frame, h, w)
