// mxv_render.hip — render_mode="rgb_array" frames of the classic-control envs, drawn on the device (include/mxv_render.h).
//
// A frame is (1) the reference's draw list, recomputed from the handle's fp64 state and physics attributes in the reference's own
// operation order (cartpole.py:209-304, acrobot.py:279-367, mountain_car.py:169-274, continuous_mountain_car.py:191-292; pygame's
// Vector2.rotate_rad restated with its fmod and 90-degree special cases; sin / cos correctly rounded, mxv_exact.hpp), turned into integer
// records by ONE rule (fix() below: int() of the pixel value, of 8 x the value for aalines points), and (2) those records rasterised with
// integer arithmetic only — 4 x 4 samples per pixel, coverage blend — so that tests/render_host.py computes the same bytes on the host.
//
// Launch shape.  One workgroup of 256 threads per (frame, band of 16 output rows).  Each workgroup rebuilds the frame's scene in LDS
// (MountainCar's 100 track points one per thread), keeps the records whose bounding box reaches its rows (ballot compaction, draw order
// kept), and writes the band as a flat byte stream: a thread owns runs of 16 pixels = 48 B = 3 dwordx4 stores (runs may straddle rows;
// 16 rows x W pixels is a whole number of runs, and every frame is a multiple of 16 B).  A band no record reaches is all white: stores
// only.  Envs whose index lies outside [0, N) get an all-zero frame and latch kRenderIndexErrorBit.
//
// pixels_kernel (below) draws the same pixels into LDS and reduces them to pixel observations (gray, area resize) without writing the
// frame (DESIGN.md §10 "Pixel observations").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "mxv_device.hpp"   // mxv_exact.hpp (correctly rounded sin / cos) and clamp_range, the clip of the Pendulum step
#include "mxv_render.hpp"
#include "../../include/mxv_render.h"

namespace mxv {
namespace render {

constexpr int kThreads = 256;
constexpr int kBandRows = 16;
constexpr int kRec = MXV_RENDER_RECORD_INTS;
constexpr int kMaxRec = MXV_RENDER_MAX_RECORDS;
constexpr int kTrack = 100;
constexpr double kLimitPx = 1048576.0;  // 2^20: coordinates beyond it (or non-finite) skip the primitive
constexpr double kTwoPi = 2 * M_PI, kHalfPi = M_PI / 2, kVectorEpsilon = 1e-6;
constexpr int64_t kMaxCount = (int64_t)1 << 24;

__host__ __device__ inline bool square_frame(int kind) { return kind == MXV_ACROBOT || kind == MXV_PENDULUM; }
__host__ __device__ inline int frame_h(int kind) { return square_frame(kind) ? 500 : 400; }
__host__ __device__ inline int frame_w(int kind) { return square_frame(kind) ? 500 : 600; }
__host__ __device__ inline int kind_records(int kind) { return kind == MXV_CARTPOLE ? 7 : square_frame(kind) ? 9 : 108; }

// (sin x, cos x): correctly rounded where mxv_exact.hpp covers the argument, the device libm beyond, NaN for non-finite x
__device__ inline void sincos_rn(double x, double *s, double *c) {
    if (fabs(x) < 524288.0) {
        exact::cr_sincos(x, s, c);
    } else if (isfinite(x)) {
        *s = sin(x);
        *c = cos(x);
    } else {
        *s = *c = NAN;
    }
}

// pygame 2.1 Vector2.rotate_rad (math.c, _vector2_rotate_helper)
__device__ inline void rotate_rad(double x, double y, double angle, double *ox, double *oy) {
    if (!isfinite(angle)) {
        *ox = *oy = NAN;
        return;
    }
    angle = fmod(angle, kTwoPi);
    if (angle < 0) angle += kTwoPi;
    if (fmod(angle + kVectorEpsilon, kHalfPi) < 2 * kVectorEpsilon) {
        switch ((int)((angle + kVectorEpsilon) / kHalfPi)) {
            case 1: *ox = -y; *oy = x; return;
            case 2: *ox = -x; *oy = -y; return;
            case 3: *ox = y; *oy = -x; return;
            default: *ox = x; *oy = y; return;
        }
    }
    double s, c;
    sincos_rn(angle, &s, &c);
    *ox = c * x - s * y;
    *oy = s * x + c * y;
}

// THE float -> integer rule (1/8-px units): int() of the pixel value times 8, or int() of 8 v (aalines); false if unrepresentable
__device__ inline bool fix(double v, bool sub, int32_t *out) {
    if (!(fabs(v) <= kLimitPx)) return false;
    *out = sub ? (int32_t)(int64_t)(v * 8.0) : (int32_t)((int64_t)v * 8);
    return true;
}

template <int N>
__device__ inline void put(int32_t *r, int op, uint32_t rgb, const double *xy, bool sub, int32_t radius = 0) {
    int32_t v[2 * N];
    bool ok = radius >= 0;
#pragma unroll
    for (int i = 0; i < 2 * N; ++i) ok = fix(xy[i], sub, &v[i]) && ok;
#pragma unroll
    for (int i = 0; i < kRec; ++i) r[i] = 0;
    if (!ok) return;
    r[0] = op;
    r[1] = (int32_t)rgb;
    r[2] = N;
    r[3] = radius;
#pragma unroll
    for (int i = 0; i < 2 * N; ++i) r[4 + i] = v[i];
}

// gfxdraw circles receive int(x), int(y), int(r): the radius passes the same rule
__device__ inline void put_circle(int32_t *r, int op, uint32_t rgb, double x, double y, double radius) {
    int32_t rr;
    if (!fix(radius, false, &rr)) {
        for (int i = 0; i < kRec; ++i) r[i] = 0;
        return;
    }
    const double xy[2] = {x, y};
    put<1>(r, op, rgb, xy, false, rr / 8);
}

__device__ inline void put_quad(int32_t *r, uint32_t rgb, const double (*c)[2]) {
    const double xy[8] = {c[0][0], c[0][1], c[1][0], c[1][1], c[2][0], c[2][1], c[3][0], c[3][1]};
    put<4>(r, MXV_RENDER_AAPOLYGON, rgb, xy, false);
    put<4>(r + kRec, MXV_RENDER_FILLED_POLYGON, rgb, xy, false);
}

__device__ inline double mc_height(double v) {
    double s, c;
    sincos_rn(3 * v, &s, &c);
    return s * 0.45 + 0.55;
}

// Pendulum's arrow (pendulum.py:235-244): smoothscale to (scale * |last_u| / 2,) * 2 — float32 arithmetic (NumPy 2 keeps the Python
// float weak), int() of the size as for every gfxdraw argument — flipped horizontally when last_u > 0 and always vertically, blitted at
// (offset - w // 2, offset - h // 2) (Rect.centerx / centery).  No record for None (NaN) or a size beyond the coordinate limit.
__device__ inline void put_blit(int32_t *r, float u, double scale, int offset) {
    for (int i = 0; i < kRec; ++i) r[i] = 0;
    const float size = (float)scale * fabsf(u) / 2.0f;
    if (!(size <= (float)kLimitPx)) return;
    const int32_t wh = (int32_t)size;
    r[0] = MXV_RENDER_BLIT;
    r[4] = offset - wh / 2;
    r[5] = offset - wh / 2;
    r[6] = wh;
    r[7] = wh;
    r[8] = u > 0.0f ? 1 : 0;
    r[9] = 1;
}

// The frame's records into rec[kMaxRec][kRec] (LDS).  Called by every thread of the block; ends with a barrier.  `u`: Pendulum's last_u.
__device__ void build_scene(int kind, const double *s, const double *P, float u, int32_t (*rec)[kRec], double *tx, double *ty) {
    const int t = threadIdx.x;
    const int nrec = kind_records(kind);
    for (int i = nrec + t; i < kMaxRec; i += blockDim.x)
        for (int j = 0; j < kRec; ++j) rec[i][j] = 0;
    if (kind == MXV_CARTPOLE) {
        if (t == 0) {
            const double length = P[4], xth = P[9];
            const double world_width = xth * 2;
            const double scale = 600.0 / world_width;
            const double polewidth = 10.0, polelen = scale * (2 * length);
            const double cartwidth = 50.0, cartheight = 30.0;
            double l = -cartwidth / 2, r = cartwidth / 2, tp = cartheight / 2, b = -cartheight / 2;
            const double axleoffset = cartheight / 4.0;
            const double cartx = s[0] * scale + 600 / 2.0;
            const double carty = 100;
            const double cart[4][2] = {{l + cartx, b + carty}, {l + cartx, tp + carty}, {r + cartx, tp + carty}, {r + cartx, b + carty}};
            put_quad(rec[0], 0x000000u, cart);
            l = -polewidth / 2, r = polewidth / 2, tp = polelen - polewidth / 2, b = -polewidth / 2;
            const double src[4][2] = {{l, b}, {l, tp}, {r, tp}, {r, b}};
            double pole[4][2];
            for (int k = 0; k < 4; ++k) {
                double cx, cy;
                rotate_rad(src[k][0], src[k][1], -s[2], &cx, &cy);
                pole[k][0] = cx + cartx;
                pole[k][1] = cy + carty + axleoffset;
            }
            put_quad(rec[2], 0xCA9865u, pole);
            put_circle(rec[4], MXV_RENDER_AACIRCLE, 0x8184CBu, cartx, carty + axleoffset, polewidth / 2);
            put_circle(rec[5], MXV_RENDER_FILLED_CIRCLE, 0x8184CBu, cartx, carty + axleoffset, polewidth / 2);
            const double hl[4] = {0, carty, 600, carty};
            put<2>(rec[6], MXV_RENDER_HLINE, 0x000000u, hl, false);
        }
    } else if (kind == MXV_ACROBOT) {
        if (t == 0) {
            const double L1 = P[1], L2 = P[2];
            const double bound = L1 + L2 + 0.2;
            const double scale = 500.0 / (bound * 2);
            const double offset = 500 / 2.0;
            double s0, c0;
            sincos_rn(s[0], &s0, &c0);
            const double p1x = -L1 * c0 * scale, p1y = L1 * s0 * scale;
            const double xys[2][2] = {{0.0, 0.0}, {p1y, p1x}};
            const double thetas[2] = {s[0] - M_PI / 2, s[0] + s[1] - M_PI / 2};
            const double link_lengths[2] = {L1 * scale, L2 * scale};
            const double ln[4] = {-2.2 * scale + offset, 1 * scale + offset, 2.2 * scale + offset, 1 * scale + offset};
            put<2>(rec[0], MXV_RENDER_LINE, 0x000000u, ln, false);
            for (int k = 0; k < 2; ++k) {
                const double x = xys[k][0] + offset, y = xys[k][1] + offset;
                const double l = 0, r = link_lengths[k], tp = 0.1 * scale, b = -0.1 * scale;
                const double src[4][2] = {{l, b}, {l, tp}, {r, tp}, {r, b}};
                double q[4][2];
                for (int j = 0; j < 4; ++j) {
                    double cx, cy;
                    rotate_rad(src[j][0], src[j][1], thetas[k], &cx, &cy);
                    q[j][0] = cx + x;
                    q[j][1] = cy + y;
                }
                put_quad(rec[1 + 4 * k], 0x00CCCCu, q);
                put_circle(rec[3 + 4 * k], MXV_RENDER_AACIRCLE, 0xCCCC00u, x, y, 0.1 * scale);
                put_circle(rec[4 + 4 * k], MXV_RENDER_FILLED_CIRCLE, 0xCCCC00u, x, y, 0.1 * scale);
            }
        }
    } else if (kind == MXV_PENDULUM) {  // pendulum.py:197-249
        if (t == 0) {
            const double bound = 2.2;
            const double scale = 500 / (bound * 2);
            const int offset = 500 / 2;
            const double rod_length = 1 * scale, rod_width = 0.2 * scale;
            const double l = 0, r = rod_length, tp = rod_width / 2, b = -rod_width / 2;
            const double src[4][2] = {{l, b}, {l, tp}, {r, tp}, {r, b}};
            const double angle = s[0] + M_PI / 2;
            double q[4][2];
            for (int j = 0; j < 4; ++j) {
                double cx, cy;
                rotate_rad(src[j][0], src[j][1], angle, &cx, &cy);
                q[j][0] = cx + offset;
                q[j][1] = cy + offset;
            }
            put_quad(rec[0], 0xCC4D4Du, q);
            put_circle(rec[2], MXV_RENDER_AACIRCLE, 0xCC4D4Du, offset, offset, rod_width / 2);
            put_circle(rec[3], MXV_RENDER_FILLED_CIRCLE, 0xCC4D4Du, offset, offset, rod_width / 2);
            double ex, ey;   // rod_end: int() of the rotated (rod_length, 0) plus the offset, then gfxdraw's int() again (a no-op)
            rotate_rad(rod_length, 0.0, angle, &ex, &ey);
            put_circle(rec[4], MXV_RENDER_AACIRCLE, 0xCC4D4Du, ex + offset, ey + offset, rod_width / 2);
            put_circle(rec[5], MXV_RENDER_FILLED_CIRCLE, 0xCC4D4Du, ex + offset, ey + offset, rod_width / 2);
            put_blit(rec[6], u, scale, offset);
            put_circle(rec[7], MXV_RENDER_AACIRCLE, 0x000000u, offset, offset, 0.05 * scale);
            put_circle(rec[8], MXV_RENDER_FILLED_CIRCLE, 0x000000u, offset, offset, 0.05 * scale);
        }
    } else {  // MountainCar-v0 (0 min_position 1 max_position 3 goal_position) / MountainCarContinuous-v0 (2, 3, 5)
        const bool cont = kind == MXV_MOUNTAINCAR_CONT;
        const double lo = cont ? P[2] : P[0], hi = cont ? P[3] : P[1], goal = cont ? P[5] : P[3];
        const double world_width = hi - lo;
        const double scale = 600.0 / world_width;
        if (t < kTrack) {  // np.linspace(lo, hi, 100): i * step + lo, the last point = hi exactly
            double px = NAN, py = NAN;
            if (isfinite(lo) && isfinite(hi)) {
                const double step = (hi - lo) / 99;
                const double xs = t == kTrack - 1 ? hi : (double)t * step + lo;
                const double ys = mc_height(xs);
                px = (xs - lo) * scale;
                py = ys * scale;
            }
            tx[t] = px;
            ty[t] = py;
        }
        __syncthreads();
        if (t < kTrack - 1) {
            const double seg[4] = {tx[t], ty[t], tx[t + 1], ty[t + 1]};
            put<2>(rec[t], MXV_RENDER_AALINE, 0x000000u, seg, true);
        }
        if (t == kTrack - 1) {
            int32_t(*r)[kRec] = rec + (kTrack - 1);
            const double carwidth = 40, carheight = 20;
            const double pos = s[0];
            const double clearance = 10;
            const double l = -carwidth / 2, rr = carwidth / 2, tp = carheight, b = 0;
            double ang = NAN;
            if (isfinite(pos)) {
                double sn;
                sincos_rn(3 * pos, &sn, &ang);
            }
            const double hp = mc_height(pos);
            const double src[4][2] = {{l, b}, {l, tp}, {rr, tp}, {rr, b}};
            double q[4][2];
            for (int j = 0; j < 4; ++j) {
                double cx, cy;
                rotate_rad(src[j][0], src[j][1], ang, &cx, &cy);
                q[j][0] = cx + (pos - lo) * scale;
                q[j][1] = cy + clearance + hp * scale;
            }
            put_quad(r[0], 0x000000u, q);
            const double wheels[2] = {carwidth / 4, -carwidth / 4};
            for (int k = 0; k < 2; ++k) {
                double cx, cy;
                rotate_rad(wheels[k], 0.0, ang, &cx, &cy);
                const double wx = cx + (pos - lo) * scale, wy = cy + clearance + hp * scale;
                put_circle(r[2 + 2 * k], MXV_RENDER_AACIRCLE, 0x808080u, wx, wy, carheight / 2.5);
                put_circle(r[3 + 2 * k], MXV_RENDER_FILLED_CIRCLE, 0x808080u, wx, wy, carheight / 2.5);
            }
            int32_t fx, fy1;
            const bool ok = fix((goal - lo) * scale, false, &fx) && fix(mc_height(goal) * scale, false, &fy1);
            if (!ok) {
                for (int k = 6; k < 9; ++k)
                    for (int j = 0; j < kRec; ++j) r[k][j] = 0;
            } else {
                const double flagx = fx / 8, flagy1 = fy1 / 8, flagy2 = flagy1 + 50;
                const double vl[4] = {flagx, flagy1, flagx, flagy2};
                put<2>(r[6], MXV_RENDER_VLINE, 0x000000u, vl, false);
                const double tri[6] = {flagx, flagy2, flagx, flagy2 - 10, flagx + 25, flagy2 - 5};
                put<3>(r[7], MXV_RENDER_AAPOLYGON, 0xCCCC00u, tri, false);
                put<3>(r[8], MXV_RENDER_FILLED_POLYGON, 0xCCCC00u, tri, false);
            }
        }
    }
    __syncthreads();
}

// -- rasterisation (integer only; tests/render_host.py states the same rule in NumPy) ------------------------------------------------
__device__ inline int64_t floor_div8(int64_t v) { return v >= 0 ? v / 8 : -((-v + 7) / 8); }

// The 16 samples of a pixel are the bits iy * 4 + ix of a mask, at (8 x + 2 ix - 3, 8 y + 2 iy - 3) in 1/8 px.
// Samples whose coordinate along one axis lies in [lo, hi]: a 4-bit mask.
__device__ inline uint32_t axis_mask(int64_t base, int64_t lo, int64_t hi) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t v = base + 2 * i - 3;
        m |= (v >= lo && v <= hi) ? 1u << i : 0u;
    }
    return m;
}

__device__ inline uint32_t box_mask(int64_t X8, int64_t Y8, int64_t xlo, int64_t xhi, int64_t ylo, int64_t yhi) {
    const uint32_t xm = axis_mask(X8, xlo, xhi), ym = axis_mask(Y8, ylo, yhi);
    uint32_t m = 0;
#pragma unroll
    for (int iy = 0; iy < 4; ++iy) m |= ((ym >> iy) & 1u) ? xm << (4 * iy) : 0u;
    return m;
}

// samples with sign * E >= -w, E = dx (sy - ay) - dy (sx - ax) the edge function of the edge from a along (dx, dy).  E at a sample is
// E(centre) + dx oy - dy ox with |dx oy - dy ox| <= 6 * 2^24 (coordinates are bounded by 2^23): the sample terms fit in int32 and the
// threshold, once it lies within their reach, too.  Pixels wholly on one side of the edge take the early exits.
__device__ inline uint32_t edge_mask(int64_t X8, int64_t Y8, int64_t ax, int64_t ay, int64_t dx, int64_t dy, int64_t w, int64_t sign) {
    const int64_t e0 = sign * (dx * (Y8 - ay) - dy * (X8 - ax));
    const int64_t thr = -w - e0;
    const int64_t reach = 3 * (llabs(dx) + llabs(dy));   // |dx oy - dy ox| over the 16 samples
    if (thr <= -reach) return 0xFFFFu;                    // every sample passes (pixel well inside the half-plane) ...
    if (thr > reach) return 0u;                           // ... or none does
    const int32_t t = (int32_t)thr;
    const int32_t sdx = (int32_t)(sign * dx), sdy = (int32_t)(sign * dy);
    uint32_t m = 0;
#pragma unroll
    for (int iy = 0; iy < 4; ++iy)
#pragma unroll
        for (int ix = 0; ix < 4; ++ix) m |= (sdx * (2 * iy - 3) - sdy * (2 * ix - 3) >= t) ? 1u << (4 * iy + ix) : 0u;
    return m;
}

// the segment a-b grown by the half-pixel square: bounding box grown by 4 and |E| <= 4 (|dx| + |dy|)
__device__ inline uint32_t seg_mask(int64_t X8, int64_t Y8, int64_t ax, int64_t ay, int64_t bx, int64_t by) {
    uint32_t m = box_mask(X8, Y8, min(ax, bx) - 4, max(ax, bx) + 4, min(ay, by) - 4, max(ay, by) + 4);
    if (!m) return 0;
    const int64_t dx = bx - ax, dy = by - ay, w = 4 * (llabs(dx) + llabs(dy));
    return m & edge_mask(X8, Y8, ax, ay, dx, dy, w, 1) & edge_mask(X8, Y8, ax, ay, dx, dy, w, -1);
}

// the triangle a b c grown by the half-pixel square: bounding box grown by 4 and s E_edge >= -4 (|dx| + |dy|) for its three edges
__device__ inline uint32_t tri_mask(int64_t X8, int64_t Y8, int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t cx, int64_t cy) {
    uint32_t m = box_mask(X8, Y8, min(min(ax, bx), cx) - 4, max(max(ax, bx), cx) + 4, min(min(ay, by), cy) - 4, max(max(ay, by), cy) + 4);
    if (!m) return 0;
    const int64_t sgn = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax) >= 0 ? 1 : -1;
    m &= edge_mask(X8, Y8, ax, ay, bx - ax, by - ay, 4 * (llabs(bx - ax) + llabs(by - ay)), sgn);
    if (!m) return 0;
    m &= edge_mask(X8, Y8, bx, by, cx - bx, cy - by, 4 * (llabs(cx - bx) + llabs(cy - by)), sgn);
    if (!m) return 0;
    return m & edge_mask(X8, Y8, cx, cy, ax - cx, ay - cy, 4 * (llabs(ax - cx) + llabs(ay - cy)), sgn);
}

// samples (of 16) of pixel (x, y) inside record r.  Not inlined: one copy of this code serves every pixel loop.
__device__ __noinline__ int coverage(const int32_t *r, int64_t x, int64_t y) {
    const int op = r[0], n = r[2];
    const int64_t x0 = r[4], y0 = r[5], x1 = r[6], y1 = r[7], x2 = r[8], y2 = r[9], x3 = r[10], y3 = r[11];
    const int64_t X8 = 8 * x, Y8 = 8 * y;
    uint32_t m = 0;
    if (op == MXV_RENDER_FILLED_POLYGON) {            // fan (v0, v1, v2), (v0, v2, v3)
        m = tri_mask(X8, Y8, x0, y0, x1, y1, x2, y2);
        if (n == 4) m |= tri_mask(X8, Y8, x0, y0, x2, y2, x3, y3);
    } else if (op == MXV_RENDER_AAPOLYGON) {          // closed outline
        m = seg_mask(X8, Y8, x0, y0, x1, y1) | seg_mask(X8, Y8, x1, y1, x2, y2);
        m |= n == 4 ? seg_mask(X8, Y8, x2, y2, x3, y3) | seg_mask(X8, Y8, x3, y3, x0, y0) : seg_mask(X8, Y8, x2, y2, x0, y0);
    } else if (op == MXV_RENDER_AACIRCLE || op == MXV_RENDER_FILLED_CIRCLE) {
        const int64_t rad = r[3];
        const int64_t outer = 8 * rad + 4, inner = max(8 * rad - 4, (int64_t)0);
#pragma unroll
        for (int iy = 0; iy < 4; ++iy)
#pragma unroll
            for (int ix = 0; ix < 4; ++ix) {
                const int64_t ddx = X8 + 2 * ix - 3 - x0, ddy = Y8 + 2 * iy - 3 - y0;
                const int64_t d2 = ddx * ddx + ddy * ddy;
                const bool in = d2 <= outer * outer && (op == MXV_RENDER_FILLED_CIRCLE || d2 >= inner * inner);
                m |= in ? 1u << (4 * iy + ix) : 0u;
            }
    } else {
        m = seg_mask(X8, Y8, x0, y0, x1, y1);
    }
    return __popc(m);
}

// pixel bounding box of record r in surface coordinates (y up), clipped: x0, x1, y0, y1 (empty: x0 > x1 or y0 > y1)
__device__ inline void record_bbox(const int32_t *r, int H, int W, int32_t *bb) {
    const int op = r[0], n = r[2];
    if (op == MXV_RENDER_NONE) {
        bb[0] = 1, bb[1] = 0, bb[2] = 1, bb[3] = 0;
        return;
    }
    if (op == MXV_RENDER_BLIT) {   // whole pixels [x, x + w) x [y, y + h); w = 0: empty
        bb[0] = max(r[4], 0), bb[1] = (int32_t)min((int64_t)r[4] + r[6] - 1, (int64_t)W - 1);
        bb[2] = max(r[5], 0), bb[3] = (int32_t)min((int64_t)r[5] + r[7] - 1, (int64_t)H - 1);
        return;
    }
    int64_t x0 = r[4], x1 = r[4], y0 = r[5], y1 = r[5];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        if (k < n) {
            x0 = min(x0, (int64_t)r[4 + 2 * k]), x1 = max(x1, (int64_t)r[4 + 2 * k]);
            y0 = min(y0, (int64_t)r[5 + 2 * k]), y1 = max(y1, (int64_t)r[5 + 2 * k]);
        }
    }
    const int64_t grow = (op == MXV_RENDER_AACIRCLE || op == MXV_RENDER_FILLED_CIRCLE) ? 8 * (int64_t)r[3] + 4 : 4;
    bb[0] = (int32_t)max(floor_div8(x0 - grow - 3), (int64_t)0);
    bb[1] = (int32_t)min(-floor_div8(-(x1 + grow + 3)), (int64_t)W - 1);
    bb[2] = (int32_t)max(floor_div8(y0 - grow - 3), (int64_t)0);
    bb[3] = (int32_t)min(-floor_div8(-(y1 + grow + 3)), (int64_t)H - 1);
}

struct RenderArgs {
    const double *state;   // [S][N]
    const double *params_pe;  // [MXV_MAX_PARAMS][N] or nullptr
    const int32_t *idx;    // [count] or nullptr (frame k = env k)
    uint8_t *frames;       // render_kernel: [count][H][W][3]
    int32_t *records;      // scene_kernel: [count][kMaxRec][kRec]
    int32_t *err;          // the render kernels' own word of the handle's latch block (pinned host memory)
    const float *last_u;   // Pendulum: [N] or nullptr (no arrow)
    const uint4 *sat;      // Pendulum: the arrow's summed-area table [img_h + 1][img_w + 1]
    int64_t n;
    int32_t kind;
    int32_t S;
    int32_t img_h, img_w;
    double P[MXV_MAX_PARAMS];
};

// The render word only ever receives this one bit: a plain store does what an atomic OR would, and no device atomic targets host memory.
__device__ __forceinline__ void raise_render_error(int32_t *err) { *reinterpret_cast<volatile int32_t *>(err) = kRenderIndexErrorBit; }

struct SceneLds {
    int32_t rec[kMaxRec][kRec];
    double tx[kTrack], ty[kTrack];
};

// the env a frame shows, its state and its attributes; false (uniform over the block) for an index outside [0, N)
__device__ inline bool load_env(const RenderArgs &a, int64_t frame, double *s, double *P, float *u) {
    const int64_t env = a.idx ? (int64_t)a.idx[frame] : frame;
    if (env < 0 || env >= a.n) return false;
    for (int k = 0; k < 4; ++k) s[k] = k < a.S ? a.state[(size_t)k * a.n + env] : 0.0;
    for (int k = 0; k < MXV_MAX_PARAMS; ++k) P[k] = a.params_pe ? a.params_pe[(size_t)k * a.n + env] : a.P[k];
    *u = a.last_u ? a.last_u[env] : NAN;
    return true;
}

__global__ __launch_bounds__(kThreads) void scene_kernel(RenderArgs a) {
    __shared__ SceneLds L;
    const int64_t frame = blockIdx.x;
    int32_t *out = a.records + (size_t)frame * kMaxRec * kRec;
    double s[4], P[MXV_MAX_PARAMS];
    float u;
    if (!load_env(a, frame, s, P, &u)) {
        if (threadIdx.x == 0) raise_render_error(a.err);
        for (int i = threadIdx.x; i < kMaxRec * kRec; i += blockDim.x) out[i] = 0;
        return;
    }
    build_scene(a.kind, s, P, u, L.rec, L.tx, L.ty);
    for (int i = threadIdx.x; i < kMaxRec * kRec; i += blockDim.x) out[i] = L.rec[i / kRec][i % kRec];
}

__device__ inline void store_run(uint4 *dst, uint32_t word) {
    const uint4 v = make_uint4(word, word, word, word);
    dst[0] = v;
    dst[1] = v;
    dst[2] = v;
}

// A workgroup's view of its scene's records: clipped pixel bounding boxes and the list of those that reach its rows, in draw order.
struct CullLds {
    int32_t bbox[kMaxRec][4];
    int32_t list[kMaxRec];
    uint64_t masks[kMaxRec / 64 + 1];
    int32_t nlist;
};

// The records whose bounding box (C.bbox, filled by threads t < kMaxRec) reaches surface rows [ylo, yhi], ballot-compacted into C.list
// in draw order; returns their number.  Called by every thread; ends with a barrier.
__device__ inline int cull_records(CullLds &C, int ylo, int yhi) {
    const int t = threadIdx.x;
    bool hit = false;
    if (t < kMaxRec) {
        const int32_t *b = C.bbox[t];
        hit = b[0] <= b[1] && b[2] <= b[3] && b[3] >= ylo && b[2] <= yhi;
    }
    const uint64_t ballot = __ballot(hit);
    const int wave = t / 64, lane = t % 64;
    if (lane == 0 && wave <= kMaxRec / 64) C.masks[wave] = ballot;
    __syncthreads();
    if (hit) {
        int pos = __popcll(ballot & ((1ull << lane) - 1));
        for (int w = 0; w < wave; ++w) pos += __popcll(C.masks[w]);
        C.list[pos] = t;
    }
    if (t == 0) {
        int total = 0;
        for (int w = 0; w <= kMaxRec / 64; ++w) total += __popcll(C.masks[w]);
        C.nlist = total;
    }
    __syncthreads();
    return C.nlist;
}

// The listed records whose box reaches columns [rx0, rx1] of surface rows [yB, yA] (a run of 16 pixels), as a bit set over the list.
__device__ inline void run_candidates(const CullLds &C, int nl, int rx0, int rx1, int yB, int yA, uint64_t *cand0, uint64_t *cand1) {
    uint64_t c0 = 0, c1 = 0;
    for (int li = 0; li < nl; ++li) {
        const int k = C.list[li];
        if (C.bbox[k][1] < rx0 || C.bbox[k][0] > rx1 || C.bbox[k][3] < yB || C.bbox[k][2] > yA) continue;
        if (li < 64)
            c0 |= 1ull << li;
        else
            c1 |= 1ull << (li - 64);
    }
    *cand0 = c0;
    *cand1 = c1;
}

// The MXV_RENDER_BLIT record r over colour 0xRRGGBB at surface pixel (x, y) inside its box (include/mxv_render.h): the scaled image's
// pixel is the rounded window mean of the straight RGBA source, four corner loads of the summed-area table; then the alpha blend.
// Not inlined: the other kinds never reach it, and it adds nothing to shade()'s registers (its arguments travel by value: a reference to
// the kernel's argument block would put a copy of that block in scratch).
__device__ __noinline__ uint32_t blit_pixel(const int32_t *r, const uint4 *sat, int32_t img_h, int32_t img_w, int x, int y, uint32_t rgb) {
    const int64_t w = r[6], h = r[7], Hs = img_h, Ws = img_w;
    int64_t row = y - r[5], col = x - r[4];
    if (r[9]) row = h - 1 - row;
    if (r[8]) col = w - 1 - col;
    const int64_t r0 = row * Hs / h, r1 = ((row + 1) * Hs + h - 1) / h;
    const int64_t c0 = col * Ws / w, c1 = ((col + 1) * Ws + w - 1) / w;
    const uint4 p = sat[r1 * (Ws + 1) + c1], q = sat[r0 * (Ws + 1) + c1], s = sat[r1 * (Ws + 1) + c0], t = sat[r0 * (Ws + 1) + c0];
    const uint32_t n = (uint32_t)((r1 - r0) * (c1 - c0));
    const uint32_t mr = (p.x - q.x - s.x + t.x + n / 2) / n, mg = (p.y - q.y - s.y + t.y + n / 2) / n;
    const uint32_t mb = (p.z - q.z - s.z + t.z + n / 2) / n, ma = (p.w - q.w - s.w + t.w + n / 2) / n;
    const uint32_t o = 255 - ma;
    const uint32_t cr = (mr * ma + ((rgb >> 16) & 255) * o + 127) / 255;
    const uint32_t cg = (mg * ma + ((rgb >> 8) & 255) * o + 127) / 255;
    const uint32_t cb = (mb * ma + (rgb & 255) * o + 127) / 255;
    return cr << 16 | cg << 8 | cb;
}

// The colour 0xRRGGBB of surface pixel (x, y): white, then every candidate record that covers samples of it blended in draw order.
// BLIT: the scene may hold Pendulum's arrow (a.sat set).  The callers pick the instance by a uniform branch on a.sat, so the other kinds
// run the loop without the blit test.
template <bool BLIT>
__device__ inline uint32_t shade(const RenderArgs &a, const SceneLds &L, const CullLds &C, uint64_t cand0, uint64_t cand1, int x, int y) {
    uint32_t cr = 255, cg = 255, cb = 255;
    for (int h = 0; h < 2; ++h)
    for (uint64_t mm = h ? cand1 : cand0; mm; mm &= mm - 1) {
        const int k = C.list[h * 64 + __ffsll((unsigned long long)mm) - 1];
        if (x < C.bbox[k][0] || x > C.bbox[k][1] || y < C.bbox[k][2] || y > C.bbox[k][3]) continue;
        const int32_t *r = L.rec[k];
        // Pendulum's arrow (its box is the image's rectangle: every pixel of it is drawn)
        if (BLIT && r[0] == MXV_RENDER_BLIT) {
            const uint32_t c = blit_pixel(r, a.sat, a.img_h, a.img_w, x, y, cr << 16 | cg << 8 | cb);
            cr = c >> 16, cg = (c >> 8) & 255, cb = c & 255;
            continue;
        }
        const int c = coverage(r, x, y);
        if (c == 0) continue;
        const uint32_t rgb = (uint32_t)r[1], o = 16 - c;
        cr = (cr * o + ((rgb >> 16) & 255) * c + 8) >> 4;
        cg = (cg * o + ((rgb >> 8) & 255) * c + 8) >> 4;
        cb = (cb * o + (rgb & 255) * c + 8) >> 4;
    }
    return cr << 16 | cg << 8 | cb;
}

// Surface rows [yB, yA] and columns [rx0, rx1] that bound the run of 16 pixels starting at flat pixel p0 of a block of rows that starts
// at output row row0 (a run may straddle two rows: then it spans every column of both).
__device__ inline void run_bounds(int H, int W, int row0, int p0, int *colA, int *yA, int *yB, int *rx0, int *rx1) {
    const int rowA = row0 + p0 / W;
    *colA = p0 % W;
    const bool straddle = *colA + 15 >= W;
    *yA = H - 1 - rowA;
    *yB = straddle ? *yA - 1 : *yA;
    *rx0 = straddle ? 0 : *colA;
    *rx1 = straddle ? W - 1 : *colA + 15;
}

template <int H, int W>
__global__ __launch_bounds__(kThreads) void render_kernel(RenderArgs a) {
    constexpr int kBands = (H + kBandRows - 1) / kBandRows;
    constexpr int64_t kFrameBytes = (int64_t)H * W * 3;
    static_assert(kFrameBytes % 16 == 0 && (kBandRows * W) % 16 == 0 && ((H % kBandRows) * W) % 16 == 0, "runs of 16 px tile every band");
    __shared__ SceneLds L;
    __shared__ CullLds C;
    __shared__ __attribute__((aligned(16))) uint8_t stage[kThreads][48];   // each thread's run of 16 pixels, as bytes
    const int64_t frame = blockIdx.x / kBands;
    const int band = (int)(blockIdx.x % kBands);
    const int row0 = band * kBandRows;
    const int rows = min(kBandRows, H - row0);
    const int runs = rows * W / 16;
    uint4 *o4 = (uint4 *)(a.frames + frame * kFrameBytes + (int64_t)row0 * W * 3);
    const int t = threadIdx.x;
    double s[4], P[MXV_MAX_PARAMS];
    float u;
    if (!load_env(a, frame, s, P, &u)) {
        if (t == 0 && band == 0) raise_render_error(a.err);
        for (int run = t; run < runs; run += kThreads) store_run(o4 + 3 * run, 0u);
        return;
    }
    build_scene(a.kind, s, P, u, L.rec, L.tx, L.ty);
    // records that reach this band's rows, in draw order (surface y of output row R is H - 1 - R)
    if (t < kMaxRec) record_bbox(L.rec[t], H, W, C.bbox[t]);
    const int nl = cull_records(C, H - row0 - rows, H - 1 - row0);
    if (nl == 0) {  // no primitive reaches these rows: white
        for (int run = t; run < runs; run += kThreads) store_run(o4 + 3 * run, 0xFFFFFFFFu);
        return;
    }
    for (int run = t; run < runs; run += kThreads) {
        int colA, yA, yB, rx0, rx1;
        run_bounds(H, W, row0, run * 16, &colA, &yA, &yB, &rx0, &rx1);
        uint64_t cand0, cand1;
        run_candidates(C, nl, rx0, rx1, yB, yA, &cand0, &cand1);
        uint4 *d = o4 + 3 * run;
        if (!(cand0 | cand1)) {
            store_run(d, 0xFFFFFFFFu);
            continue;
        }
        uint8_t *mine = stage[t];
#pragma nounroll
        for (int j = 0; j < 16; ++j) {
            int x = colA + j, y = yA;
            if (x >= W) x -= W, y -= 1;
            const uint32_t c = a.sat ? shade<true>(a, L, C, cand0, cand1, x, y) : shade<false>(a, L, C, cand0, cand1, x, y);
            mine[3 * j] = (uint8_t)(c >> 16);
            mine[3 * j + 1] = (uint8_t)(c >> 8);
            mine[3 * j + 2] = (uint8_t)c;
        }
        const uint4 *src = (const uint4 *)mine;
        d[0] = src[0];
        d[1] = src[1];
        d[2] = src[2];
    }
}

// -- pixel observations: render -> gray -> area resize in one pass (include/mxv_render.h mxv_pixels*, tests/pixels_host.py) --------
constexpr int kMaxOutRow = 600 * 3;       // bytes of one output row at most (w <= W, channels <= 3)
constexpr int kMaxBandBytes = 4 * kMaxOutRow;   // output bytes of one workgroup at most (its LDS stage)

// Source rows one LDS tile holds: RGB triplets 16 rows (28.8 KB at W = 600, three workgroups per CU); gray bytes 48 rows at W = 600
// (28.8 KB: 84-row observations in bands of 8 rows, 11 scene builds per frame) and 32 at W = 500, where 84 output rows make bands of
// 4 rows either way and the smaller tile keeps four workgroups per CU.
__host__ __device__ constexpr int tile_rows(int C, int W) { return C == 3 ? 16 : W == 600 ? 48 : 32; }

struct PixelArgs {
    RenderArgs r;           // state, attributes, indices, error word, N, kind (frames / records unused)
    const uint8_t *mask;    // [frames] or nullptr: frames whose byte is 0 are skipped
    uint8_t *out;           // frame k, copy c at out + k * env_stride + c * copy_stride: uint8 [h][w][channels]
    int64_t env_stride, copy_stride;
    int32_t h, w, copies;
    int32_t band_rows;      // output rows per workgroup
    int32_t bands;          // workgroups per frame
};

template <int C>
__device__ inline void tile_put(uint8_t *tile, int p, uint32_t rgb) {
    if (C == 1) {
        tile[p] = (uint8_t)((4899u * (rgb >> 16) + 9617u * ((rgb >> 8) & 255u) + 1868u * (rgb & 255u) + 8192u) >> 14);
    } else {
        tile[3 * p] = (uint8_t)(rgb >> 16);
        tile[3 * p + 1] = (uint8_t)(rgb >> 8);
        tile[3 * p + 2] = (uint8_t)rgb;
    }
}

// The band's nb output bytes (src: the LDS stage, or nullptr for `fill` everywhere) into every copy of the frame: a thread owns runs of
// 16 bytes, one dwordx4 store per copy where the destination is 16-byte aligned, byte stores elsewhere.
__device__ inline void store_band(const PixelArgs &a, uint8_t *dst0, int nb, const uint8_t *src, uint8_t fill) {
    const uint32_t f4 = fill * 0x01010101u;
    for (int g = threadIdx.x; 16 * g < nb; g += kThreads) {
        const int n = min(16, nb - 16 * g);
        uint8_t *dst = dst0 + 16 * g;
        for (int c = 0; c < a.copies; ++c, dst += a.copy_stride) {
            if (n == 16 && ((uintptr_t)dst & 15) == 0)
                *(uint4 *)dst = src ? *(const uint4 *)(src + 16 * g) : make_uint4(f4, f4, f4, f4);
            else
                for (int k = 0; k < n; ++k) dst[k] = src ? src[16 * g + k] : fill;
        }
    }
}

// One workgroup of 256 threads per (frame, band of a.band_rows output rows).  The band's source rows are rasterised exactly as
// render_kernel draws them (run_bounds, run_candidates, shade), chunk by chunk into an LDS tile with gray already applied; then one
// thread per output byte sums its source block (the rows of it inside the chunk) and the band leaves through an LDS stage in 16-byte
// stores.  A band whose source rows no record reaches is white without coverage work, and so is every run of 16 source pixels that no
// record's box reaches.  A band that needs more source rows than one tile holds (h < H / tile rows: then a band is one output row)
// keeps its running sums in LDS between chunks.
template <int H, int W, int C>
__global__ __launch_bounds__(kThreads) void pixels_kernel(PixelArgs a) {
    constexpr int kRows = tile_rows(C, W);
    static_assert(W * C <= kMaxOutRow, "one output row must fit the running sums (acc) and a band of four rows the stage");
    __shared__ SceneLds L;
    __shared__ CullLds Cl;
    __shared__ __attribute__((aligned(16))) uint8_t tile[kRows * W * C];
    __shared__ uint32_t acc[kMaxOutRow];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kMaxBandBytes];
    const int64_t frame = blockIdx.x / a.bands;
    const int band = (int)(blockIdx.x % a.bands);
    if (a.mask && a.mask[frame] == 0) return;
    const int t = threadIdx.x;
    const int h = a.h, w = a.w, rowb = w * C;
    const int i0 = band * a.band_rows, i1 = min(h, i0 + a.band_rows);
    const int nb = (i1 - i0) * rowb;                               // the band's output bytes (<= kMaxBandBytes, checked by the launch)
    uint8_t *dst0 = a.out + frame * a.env_stride + (int64_t)i0 * rowb;
    double s[4], P[MXV_MAX_PARAMS];
    float u;
    if (!load_env(a.r, frame, s, P, &u)) {
        if (t == 0 && band == 0) raise_render_error(a.r.err);
        store_band(a, dst0, nb, nullptr, 0);
        return;
    }
    build_scene(a.r.kind, s, P, u, L.rec, L.tx, L.ty);
    if (t < kMaxRec) record_bbox(L.rec[t], H, W, Cl.bbox[t]);
    const int r0 = (int)((int64_t)i0 * H / h), r1 = (int)(((int64_t)i1 * H + h - 1) / h);   // the band's source rows [r0, r1)
    const int chunks = (r1 - r0 + kRows - 1) / kRows;
    for (int q = 0; q < chunks; ++q) {
        const int s0 = r0 + q * kRows, s1 = min(r1, s0 + kRows);
        __syncthreads();                                           // the previous chunk's readers of the tile and the list are done
        const int nl = cull_records(Cl, H - s1, H - 1 - s0);
        if (nl == 0 && chunks == 1) {                              // no primitive reaches the band's source rows: white
            store_band(a, dst0, nb, nullptr, 255);
            return;
        }
        const int npix = (s1 - s0) * W;
        for (int run = t; 16 * run < npix; run += kThreads) {
            const int p0 = run * 16, n = min(16, npix - p0);
            int colA, yA, yB, rx0, rx1;
            run_bounds(H, W, s0, p0, &colA, &yA, &yB, &rx0, &rx1);
            uint64_t cand0 = 0, cand1 = 0;
            if (nl) run_candidates(Cl, nl, rx0, rx1, yB, yA, &cand0, &cand1);
            if (!(cand0 | cand1) && n == 16) {
                const uint4 white = make_uint4(~0u, ~0u, ~0u, ~0u);
#pragma unroll
                for (int k = 0; k < C; ++k) ((uint4 *)(tile + C * p0))[k] = white;
                continue;
            }
#pragma nounroll
            for (int j = 0; j < n; ++j) {
                int x = colA + j, y = yA;
                if (x >= W) x -= W, y -= 1;
                const uint32_t rgb = !(cand0 | cand1) ? 0xFFFFFFu
                                   : a.r.sat ? shade<true>(a.r, L, Cl, cand0, cand1, x, y) : shade<false>(a.r, L, Cl, cand0, cand1, x, y);
                tile_put<C>(tile, p0 + j, rgb);
            }
        }
        __syncthreads();
        // output byte b: the sum over the rows of its source block inside this chunk; the rounded mean after the last chunk
        for (int b = t; b < nb; b += kThreads) {
            const int i = i0 + b / rowb, j = (b % rowb) / C, ch = b % C;
            const int rlo = (int)((int64_t)i * H / h), rhi = (int)(((int64_t)(i + 1) * H + h - 1) / h);
            const int clo = (int)((int64_t)j * W / w), chi = (int)(((int64_t)(j + 1) * W + w - 1) / w);
            uint32_t sum = 0;
            for (int rr = max(rlo, s0); rr < min(rhi, s1); ++rr) {
                const uint8_t *row = tile + (rr - s0) * W * C + ch;
                for (int cc = clo; cc < chi; ++cc) sum += row[cc * C];
            }
            if (chunks > 1) {                                      // one output row per band: nb <= kMaxOutRow
                sum += q == 0 ? 0u : acc[b];
                acc[b] = sum;
            }
            const uint32_t cnt = (uint32_t)(rhi - rlo) * (uint32_t)(chi - clo);
            if (q + 1 == chunks) stage[b] = (uint8_t)((sum + cnt / 2) / cnt);
        }
    }
    __syncthreads();
    store_band(a, dst0, nb, stage, 0);
}

template <int H, int W>
void launch_pixels_kind(const PixelArgs &a, int C, dim3 grid, hipStream_t stream) {
    if (C == 1)
        hipLaunchKernelGGL((pixels_kernel<H, W, 1>), grid, dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((pixels_kernel<H, W, 3>), grid, dim3(kThreads), 0, stream, a);
}

RenderArgs render_args(const RenderView &v, const int32_t *idx_dev) {
    RenderArgs a{};
    a.state = v.state;
    a.params_pe = v.params_pe;
    a.idx = idx_dev;
    a.err = v.err;
    a.n = v.n;
    a.kind = v.env_id;
    a.S = v.env_id == MXV_ACROBOT || v.env_id == MXV_CARTPOLE ? 4 : 2;
    a.last_u = v.last_u;
    a.sat = v.sat;
    a.img_h = v.img_h;
    a.img_w = v.img_w;
    std::memcpy(a.P, v.P, sizeof a.P);
    return a;
}

int launch(const RenderView &v, const int32_t *idx_dev, int64_t count, uint8_t *frames, int32_t *records) {
    RenderArgs a = render_args(v, idx_dev);
    a.frames = frames;
    a.records = records;
    if (records) {
        hipLaunchKernelGGL(scene_kernel, dim3((unsigned)count), dim3(kThreads), 0, v.stream, a);
    } else if (square_frame(v.env_id)) {   // Acrobot, Pendulum
        hipLaunchKernelGGL((render_kernel<500, 500>), dim3((unsigned)(count * ((500 + kBandRows - 1) / kBandRows))), dim3(kThreads), 0,
                           v.stream, a);
    } else {
        hipLaunchKernelGGL((render_kernel<400, 600>), dim3((unsigned)(count * ((400 + kBandRows - 1) / kBandRows))), dim3(kThreads), 0,
                           v.stream, a);
    }
    return hipGetLastError() == hipSuccess ? MXV_OK : MXV_ERR_HIP;
}

// Output rows per workgroup: as many as keep the band's source rows inside one tile (at least one) and its bytes inside the LDS stage,
// rounded down to a multiple that starts every band on a 16-byte boundary of the frame where that still leaves one row or more.
int pixel_band_rows(int H, int W, int h, int w, int C) {
    const int rowb = w * C;
    int R = std::max(1, (tile_rows(C, W) - 2) * h / H);
    R = std::min(R, kMaxBandBytes / rowb);
    int g = 16;
    while (rowb % g) g /= 2;
    const int align = 16 / g;
    if (R >= align) R -= R % align;
    return R;
}

int launch_pixels(const RenderView &v, const int32_t *idx_dev, const uint8_t *mask_dev, int64_t frames, int32_t height, int32_t width,
                  int32_t channels, int32_t copies, uint8_t *out, int64_t env_stride, int64_t copy_stride) {
    PixelArgs a{};
    a.r = render_args(v, idx_dev);
    a.mask = mask_dev;
    a.out = out;
    a.env_stride = env_stride;
    a.copy_stride = copy_stride;
    a.h = height;
    a.w = width;
    a.copies = copies;
    const int H = frame_h(v.env_id);
    a.band_rows = pixel_band_rows(H, frame_w(v.env_id), height, width, channels);
    a.bands = (height + a.band_rows - 1) / a.band_rows;
    const dim3 grid((unsigned)(frames * a.bands));
    if (square_frame(v.env_id))
        launch_pixels_kind<500, 500>(a, channels, grid, v.stream);
    else
        launch_pixels_kind<400, 600>(a, channels, grid, v.stream);
    return hipGetLastError() == hipSuccess ? MXV_OK : MXV_ERR_HIP;
}

bool renderable(int32_t env_id) {
    return env_id == MXV_CARTPOLE || env_id == MXV_ACROBOT || env_id == MXV_MOUNTAINCAR || env_id == MXV_MOUNTAINCAR_CONT;
}

int check_args(mxv_handle *h, int64_t count, bool have_idx, const void *out) {
    if (!h) return MXV_ERR_INVALID_ARG;
    if (!out) return render_fail(h, MXV_ERR_INVALID_ARG, "render: output pointer is NULL");
    if (count <= 0 || count > kMaxCount) return render_fail(h, MXV_ERR_INVALID_ARG, "render: count must lie in [1, 2^24]");
    return MXV_OK;
}

// the handle's view after the checks that need its size / kind (count > N without indices, unsupported kinds)
int view_for(mxv_handle *h, int64_t count, bool have_idx, RenderView *v) {
    if (!render_ready(h))
        return render_fail(h, MXV_ERR_UNSUPPORTED, "render: Pendulum-v1 draws an image asset (pendulum.py:228-244) that the engine does not "
                                                   "carry: no rgb_array frames for it until the caller attaches one (mxv_render_attach_image)");
    if (int rc = render_view(h, v)) return rc;
    if (!have_idx && count > v->n) return render_fail(h, MXV_ERR_INVALID_ARG, "render: count > num_envs without an index list");
    return MXV_OK;
}

struct DeviceBuffer {
    void *p = nullptr;
    ~DeviceBuffer() {
        if (p) (void)hipFree(p);
    }
};

// -- Pendulum's arrow: the image's summed-area table and the per-env last_u ----------------------------------------------------------
constexpr int kTableThreads = 1024;

// sat[i][j] = per-channel sums of rgba over rows < i, columns < j (uint32: 1024 x 1024 x 255 < 2^32).  One workgroup: row prefixes, then
// column prefixes, one thread per row / column.
__global__ __launch_bounds__(kTableThreads) void blit_table_kernel(const uint8_t *rgba, uint4 *sat, int32_t h, int32_t w) {
    const int64_t ld = (int64_t)w + 1;
    for (int j = threadIdx.x; j <= w; j += blockDim.x) sat[j] = make_uint4(0, 0, 0, 0);
    for (int i = threadIdx.x; i < h; i += blockDim.x) {
        uint4 run = make_uint4(0, 0, 0, 0);
        sat[(i + 1) * ld] = run;
        for (int j = 0; j < w; ++j) {
            const uint8_t *p = rgba + ((int64_t)i * w + j) * 4;
            run.x += p[0], run.y += p[1], run.z += p[2], run.w += p[3];
            sat[(i + 1) * ld + j + 1] = run;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < w; j += blockDim.x) {
        uint4 run = make_uint4(0, 0, 0, 0);
        for (int i = 1; i <= h; ++i) {
            const uint4 v = sat[i * ld + j + 1];
            run.x += v.x, run.y += v.y, run.z += v.z, run.w += v.w;
            sat[i * ld + j + 1] = run;
        }
    }
}

constexpr int kTrackThreads = 256;

__global__ __launch_bounds__(kTrackThreads) void track_reset_kernel(float *last_u, const uint8_t *mask, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kTrackThreads + threadIdx.x;
    if (i < n && (!mask || mask[i])) last_u[i] = NAN;
}

// The clip of Env<MXV_PENDULUM>::step (the same clamp_range of mxv_device.hpp: IEEE maximum / minimum, NaN passes through, -0 < +0), then
// None where the step's autoreset ran (elapsed == 0 after a step happens only there).
__global__ __launch_bounds__(kTrackThreads) void track_step_kernel(float *last_u, const float *actions, const void *elapsed, int32_t el16,
                                                                  const double *params_pe, double max_torque, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kTrackThreads + threadIdx.x;
    if (i >= n) return;
    const double mt = params_pe ? params_pe[n + i] : max_torque;
    const float lo = (float)(-mt), hi = (float)mt;
    const float u = clamp_range(actions[i], lo, hi);
    const int32_t el = el16 ? (int32_t) static_cast<const uint16_t *>(elapsed)[i] : static_cast<const int32_t *>(elapsed)[i];
    last_u[i] = el == 0 ? NAN : u;
}

}  // namespace render

hipError_t launch_blit_table(const uint8_t *rgba, uint4 *sat, int32_t h, int32_t w, hipStream_t stream) {
    hipLaunchKernelGGL(render::blit_table_kernel, dim3(1), dim3(render::kTableThreads), 0, stream, rgba, sat, h, w);
    return hipGetLastError();
}

hipError_t launch_track_reset(float *last_u, const uint8_t *mask, int64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(render::track_reset_kernel, dim3((unsigned)((n + render::kTrackThreads - 1) / render::kTrackThreads)),
                       dim3(render::kTrackThreads), 0, stream, last_u, mask, n);
    return hipGetLastError();
}

hipError_t launch_track_step(float *last_u, const float *actions, const void *elapsed, int32_t elapsed16, const double *params_pe,
                             double max_torque, int64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(render::track_step_kernel, dim3((unsigned)((n + render::kTrackThreads - 1) / render::kTrackThreads)),
                       dim3(render::kTrackThreads), 0, stream, last_u, actions, elapsed, elapsed16, params_pe, max_torque, n);
    return hipGetLastError();
}

}  // namespace mxv

using namespace mxv;
using namespace mxv::render;

extern "C" {

int mxv_render_dims(int32_t env_id, int32_t *height, int32_t *width) {
    if (env_id < 0 || env_id >= MXV_NUM_ENV_KINDS || !height || !width) return MXV_ERR_INVALID_ARG;
    if (!renderable(env_id)) return MXV_ERR_UNSUPPORTED;
    *height = frame_h(env_id);
    *width = frame_w(env_id);
    return MXV_OK;
}

int mxv_render(mxv_handle *h, const int32_t *indices_dev, int64_t count, uint8_t *frames_dev) {
    if (int rc = check_args(h, count, indices_dev != nullptr, frames_dev)) return rc;
    if ((uintptr_t)frames_dev & 15) return render_fail(h, MXV_ERR_INVALID_ARG, "render: frames pointer is not 16-byte aligned");
    if ((uintptr_t)indices_dev & 3) return render_fail(h, MXV_ERR_INVALID_ARG, "render: index pointer is not 4-byte aligned");
    RenderView v;
    if (int rc = view_for(h, count, indices_dev != nullptr, &v)) return rc;
    if (launch(v, indices_dev, count, frames_dev, nullptr) != MXV_OK) return render_fail(h, MXV_ERR_HIP, "render: kernel launch failed");
    return MXV_OK;
}

static int render_to_host(mxv_handle *h, const int32_t *indices_host, int64_t count, void *out_host, bool scene) {
    if (int rc = check_args(h, count, indices_host != nullptr, out_host)) return rc;
    RenderView v;
    if (int rc = view_for(h, count, indices_host != nullptr, &v)) return rc;
    const size_t each = scene ? (size_t)kMaxRec * kRec * sizeof(int32_t) : (size_t)frame_h(v.env_id) * frame_w(v.env_id) * 3;
    const size_t bytes = each * (size_t)count;
    DeviceBuffer out, idx;
    if (hipMalloc(&out.p, bytes) != hipSuccess) return render_fail(h, MXV_ERR_HIP, "render: hipMalloc of the frame buffer failed");
    if (indices_host) {
        if (hipMalloc(&idx.p, (size_t)count * sizeof(int32_t)) != hipSuccess ||
            hipMemcpyAsync(idx.p, indices_host, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, v.stream) != hipSuccess)
            return render_fail(h, MXV_ERR_HIP, "render: staging the index list failed");
    }
    if (launch(v, (const int32_t *)idx.p, count, scene ? nullptr : (uint8_t *)out.p, scene ? (int32_t *)out.p : nullptr) != MXV_OK)
        return render_fail(h, MXV_ERR_HIP, "render: kernel launch failed");
    if (hipMemcpyAsync(out_host, out.p, bytes, hipMemcpyDeviceToHost, v.stream) != hipSuccess ||
        hipStreamSynchronize(v.stream) != hipSuccess)
        return render_fail(h, MXV_ERR_HIP, "render: copying the frames back failed");
    return mxv_sync(h);  // reports an index outside [0, N)
}

int mxv_render_host(mxv_handle *h, const int32_t *indices_host, int64_t count, uint8_t *frames_host) {
    return render_to_host(h, indices_host, count, frames_host, false);
}

int mxv_render_scene_host(mxv_handle *h, const int32_t *indices_host, int64_t count, int32_t *records_host) {
    return render_to_host(h, indices_host, count, records_host, true);
}

// -- pixel observations ----------------------------------------------------------------------------------------------------------------
// The kind, then the target size, channels and copies: before any device work.
static int pixel_args(mxv_handle *h, int32_t height, int32_t width, int32_t channels, int32_t copies) {
    const int32_t kind = render_env_id(h);
    if (!render_ready(h))
        return render_fail(h, MXV_ERR_UNSUPPORTED, "pixels: Pendulum-v1 draws an image asset (pendulum.py:228-244) that the engine does "
                                                   "not carry: no frames for it until the caller attaches one (mxv_render_attach_image)");
    if (channels != 1 && channels != 3) return render_fail(h, MXV_ERR_INVALID_ARG, "pixels: channels must be 1 (gray) or 3 (RGB)");
    if (height < 1 || height > frame_h(kind) || width < 1 || width > frame_w(kind))
        return render_fail(h, MXV_ERR_INVALID_ARG, "pixels: height / width must lie in [1, frame height / width]");
    if (copies < 1) return render_fail(h, MXV_ERR_INVALID_ARG, "pixels: copies must be >= 1");
    return MXV_OK;
}

static int pixels_launch(mxv_handle *h, const RenderView &v, const int32_t *idx, const uint8_t *mask, int64_t frames, int32_t height,
                         int32_t width, int32_t channels, int32_t copies, uint8_t *out, int64_t env_stride, int64_t copy_stride) {
    const int rows = pixel_band_rows(frame_h(v.env_id), frame_w(v.env_id), height, width, channels), bands = (height + rows - 1) / rows;
    if (frames * bands > (int64_t)UINT32_MAX / kThreads)
        return render_fail(h, MXV_ERR_INVALID_ARG, "pixels: too many frames for one launch at this size");
    if (launch_pixels(v, idx, mask, frames, height, width, channels, copies, out, env_stride, copy_stride) != MXV_OK)
        return render_fail(h, MXV_ERR_HIP, "pixels: kernel launch failed");
    return MXV_OK;
}

int mxv_pixels(mxv_handle *h, const int32_t *indices_dev, int64_t count, int32_t height, int32_t width, int32_t channels,
               uint8_t *out_dev) {
    if (int rc = check_args(h, count, indices_dev != nullptr, out_dev)) return rc;
    if ((uintptr_t)out_dev & 15) return render_fail(h, MXV_ERR_INVALID_ARG, "pixels: output pointer is not 16-byte aligned");
    if ((uintptr_t)indices_dev & 3) return render_fail(h, MXV_ERR_INVALID_ARG, "pixels: index pointer is not 4-byte aligned");
    if (int rc = pixel_args(h, height, width, channels, 1)) return rc;
    RenderView v;
    if (int rc = view_for(h, count, indices_dev != nullptr, &v)) return rc;
    const int64_t frame = (int64_t)height * width * channels;
    return pixels_launch(h, v, indices_dev, nullptr, count, height, width, channels, 1, out_dev, frame, 0);
}

int mxv_pixels_strided(mxv_handle *h, const uint8_t *mask_dev, int32_t height, int32_t width, int32_t channels, int32_t copies,
                       uint8_t *out_dev, int64_t env_stride, int64_t copy_stride) {
    if (!h) return MXV_ERR_INVALID_ARG;
    if (!out_dev) return render_fail(h, MXV_ERR_INVALID_ARG, "pixels: output pointer is NULL");
    if (int rc = pixel_args(h, height, width, channels, copies)) return rc;
    const int64_t frame = (int64_t)height * width * channels;
    if (env_stride < frame || (copies > 1 && copy_stride < frame))
        return render_fail(h, MXV_ERR_INVALID_ARG, "pixels: env_stride (and copy_stride when copies > 1) must be >= height * width * channels");
    RenderView v;
    if (int rc = view_for(h, 1, false, &v)) return rc;
    return pixels_launch(h, v, nullptr, mask_dev, v.n, height, width, channels, copies, out_dev, env_stride, copy_stride);
}

int mxv_pixels_host(mxv_handle *h, const int32_t *indices_host, int64_t count, int32_t height, int32_t width, int32_t channels,
                    uint8_t *out_host) {
    if (int rc = check_args(h, count, indices_host != nullptr, out_host)) return rc;
    if (int rc = pixel_args(h, height, width, channels, 1)) return rc;
    RenderView v;
    if (int rc = view_for(h, count, indices_host != nullptr, &v)) return rc;
    const int64_t frame = (int64_t)height * width * channels;
    const size_t bytes = (size_t)frame * (size_t)count;
    DeviceBuffer out, idx;
    if (hipMalloc(&out.p, bytes) != hipSuccess) return render_fail(h, MXV_ERR_HIP, "pixels: hipMalloc of the output buffer failed");
    if (indices_host) {
        if (hipMalloc(&idx.p, (size_t)count * sizeof(int32_t)) != hipSuccess ||
            hipMemcpyAsync(idx.p, indices_host, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, v.stream) != hipSuccess)
            return render_fail(h, MXV_ERR_HIP, "pixels: staging the index list failed");
    }
    if (int rc = pixels_launch(h, v, (const int32_t *)idx.p, nullptr, count, height, width, channels, 1, (uint8_t *)out.p, frame, 0))
        return rc;
    if (hipMemcpyAsync(out_host, out.p, bytes, hipMemcpyDeviceToHost, v.stream) != hipSuccess || hipStreamSynchronize(v.stream) != hipSuccess)
        return render_fail(h, MXV_ERR_HIP, "pixels: copying the frames back failed");
    return mxv_sync(h);  // reports an index outside [0, N)
}

}  // extern "C"
