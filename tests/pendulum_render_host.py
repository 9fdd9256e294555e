"""Host restatement of Pendulum-v1's frame on the engine (include/mxv_render.h MXV_RENDER_BLIT), in NumPy.

Not a test module: tests/test_pendulum_render_host.py (CPU) and tests/test_gpu_pendulum_render.py (device) import it.  It builds on
tests/render_host.py (the integer rule, the coverage rasteriser) and tests/pixels_host.py (the reduction), both unchanged.

Scene (pendulum.py:197-249): rod (aapolygon + filled_polygon), pivot circles, rod-end circles at int() of the rotated rod end, the arrow
blit when last_u is not None (NaN), the axle circles; 9 records.  The arrow record is (9, 0, 0, 0, x, y, w, h, flip_x, flip_y, 0, 0) in
whole surface pixels: w = h = int(float32(scale) * |last_u| / 2) in float32 arithmetic, x = y = 250 - w // 2, flip_x = last_u > 0,
flip_y = 1.

Blit: surface pixel (px, py) in the rectangle shows the scaled image's (r, c) = (py - y, px - x) (r -> h - 1 - r when flip_y, c ->
w - 1 - c when flip_x): the rounded mean (sum + n // 2) // n of each straight-RGBA channel over the source window of rows
[floor(r Hs / h), ceil((r + 1) Hs / h)) x columns likewise; blended as (s a + d (255 - a) + 127) // 255 with a the mean alpha.
"""
from __future__ import annotations

import math
import os

import numpy as np

import pixels_host as ph
import render_host as rh

OP_BLIT = 9
H = W = 500
RECORDS = 9
FPS = 30
SCALE = 500 / (2.2 * 2)
OFFSET = 250
ROD = (204, 77, 77)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def arrow() -> np.ndarray:
    """The fixture tests/golden/clockwise.png (the reference's asset), decoded: uint8 (312, 329, 4)."""
    from gym_amd.arrow import pendulum_arrow_image

    return pendulum_arrow_image(os.path.join(GOLDEN, "clockwise.png"))


def blit_size(u) -> int:
    """int() of scale * |last_u| / 2 in float32 (NumPy 2: the Python float is weak); -1 when the size is not representable."""
    with np.errstate(all="ignore"):
        v = np.float32(SCALE) * np.abs(np.float32(u)) / np.float32(2)
    if not (v <= rh.LIMIT_PX):
        return -1
    return int(v)


def blit_record(u) -> np.ndarray:
    out = np.zeros(rh.REC, np.int64)
    if math.isnan(float(u)):
        return out
    wh = blit_size(u)
    if wh < 0:
        return out
    out[0] = OP_BLIT
    out[4] = out[5] = OFFSET - wh // 2
    out[6] = out[7] = wh
    out[8] = 1 if float(u) > 0 else 0
    out[9] = 1
    return out


def scene(state, last_u) -> np.ndarray:
    """Records [9, 12] int64 of one frame."""
    th = float(state[0])
    nan2 = (math.nan, math.nan)

    def rot(x, y, a):
        return rh.rotate_rad(x, y, a) if math.isfinite(a) else nan2

    rod_length, rod_width = 1 * SCALE, 0.2 * SCALE
    l, r, t, b = 0, rod_length, rod_width / 2, -rod_width / 2
    angle = th + np.pi / 2
    q = []
    for cx, cy in ((l, b), (l, t), (r, t), (r, b)):
        x, y = rot(cx, cy, angle)
        q.append((x + OFFSET, y + OFFSET))
    ex, ey = rot(rod_length, 0, angle)
    recs = [rh.record(rh.OP_AAPOLYGON, ROD, q), rh.record(rh.OP_FILLED_POLYGON, ROD, q),
            rh.circle(rh.OP_AACIRCLE, ROD, OFFSET, OFFSET, rod_width / 2), rh.circle(rh.OP_FILLED_CIRCLE, ROD, OFFSET, OFFSET, rod_width / 2),
            rh.circle(rh.OP_AACIRCLE, ROD, ex + OFFSET, ey + OFFSET, rod_width / 2),
            rh.circle(rh.OP_FILLED_CIRCLE, ROD, ex + OFFSET, ey + OFFSET, rod_width / 2),
            blit_record(last_u),
            rh.circle(rh.OP_AACIRCLE, (0, 0, 0), OFFSET, OFFSET, 0.05 * SCALE),
            rh.circle(rh.OP_FILLED_CIRCLE, (0, 0, 0), OFFSET, OFFSET, 0.05 * SCALE)]
    return np.array(recs, np.int64)


def golden_records(g, i: int) -> np.ndarray:
    """The reference's recorded draw list of golden case i (tests/golden/render_pendulum.npz) after the integer rule.  Where render()
    raised (a non-finite rod end) the calls it never made are the engine's: rod-end circles skipped, arrow and axle drawn."""
    recs = []
    for j in range(8):
        op = int(g["ops"][i, j])
        color, n, pts = g["color"][i, j], int(g["npts"][i, j]), g["pts"][i, j]
        if op == 0:
            recs.append(np.zeros(rh.REC, np.int64))
        elif op in (rh.OP_AACIRCLE, rh.OP_FILLED_CIRCLE):
            recs.append(rh.circle(op, color, pts[0][0], pts[0][1], pts[1][0]))
        else:
            recs.append(rh.record(op, color, [tuple(p) for p in pts[:n]]))
    b = g["blit"][i]
    blit = np.zeros(rh.REC, np.int64)
    if b[0]:
        blit[0], blit[4:10] = OP_BLIT, b[1:7]
    if g["raised"][i]:
        tail = scene(g["states"][i], g["last_u"][i])
        blit = tail[6]
        recs[6:8] = [tail[7], tail[8]]
    recs.insert(6, blit)
    return np.array(recs, np.int64)


def window_means(img: np.ndarray, h: int, w: int) -> np.ndarray:
    """uint8 [h, w, 4]: the rounded integer mean of each channel over adaptive_avg_pool2d's windows (any h, w >= 1)."""
    Hs, Ws = img.shape[:2]
    sat = np.zeros((Hs + 1, Ws + 1, 4), np.int64)
    sat[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    rows, cols = np.array(ph.windows(Hs, h)), np.array(ph.windows(Ws, w))
    r0, r1 = rows[:, 0][:, None], rows[:, 1][:, None]
    c0, c1 = cols[:, 0][None, :], cols[:, 1][None, :]
    s = sat[r1, c1] - sat[r0, c1] - sat[r1, c0] + sat[r0, c0]
    n = ((r1 - r0) * (c1 - c0))[..., None]
    return ((s + n // 2) // n).astype(np.uint8)


def rasterize(records, img: np.ndarray) -> np.ndarray:
    """uint8 [500, 500, 3], row 0 at the top: render_host's rasteriser with the blit in its draw-order place."""
    surf = np.full((H, W, 3), 255, np.int64)   # [y][x], surface y before the flip
    for rec in records:
        op = int(rec[0])
        if op == rh.OP_NONE:
            continue
        if op == OP_BLIT:
            x, y, w, h, fx, fy = (int(v) for v in rec[4:10])
            if w <= 0 or h <= 0:
                continue
            scaled = window_means(img, h, w)
            if fy:
                scaled = scaled[::-1]
            if fx:
                scaled = scaled[:, ::-1]
            x0, x1, y0, y1 = max(x, 0), min(x + w, W), max(y, 0), min(y + h, H)
            if x0 >= x1 or y0 >= y1:
                continue
            s = scaled[y0 - y:y1 - y, x0 - x:x1 - x].astype(np.int64)
            a = s[..., 3:4]
            blk = surf[y0:y1, x0:x1]
            surf[y0:y1, x0:x1] = (s[..., :3] * a + blk * (255 - a) + 127) // 255
            continue
        x0, x1, y0, y1 = rh._bbox(rec, H, W)
        if x0 > x1 or y0 > y1:
            continue
        Y, X = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
        c = rh.coverage(rec, X, Y)[..., None]
        col = np.array([(int(rec[1]) >> 16) & 255, (int(rec[1]) >> 8) & 255, int(rec[1]) & 255], np.int64)
        blk = surf[y0:y1 + 1, x0:x1 + 1]
        surf[y0:y1 + 1, x0:x1 + 1] = (blk * (16 - c) + col * c + 8) >> 4
    return surf[::-1].astype(np.uint8)


def render(state, last_u, img: np.ndarray) -> np.ndarray:
    return rasterize(scene(state, last_u), img)


def clip(action, max_torque) -> np.float32:
    """np.clip(u, -max_torque, max_torque)[0] in float32 (pendulum.py:127): NaN stays NaN."""
    a = np.float32(action)
    lo, hi = np.float32(-max_torque), np.float32(max_torque)
    if np.isnan(a):
        return a
    return np.float32(min(max(a, lo), hi))
