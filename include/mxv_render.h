/* mxv_render.h — OPTIONAL frame rendering: render_mode="rgb_array" of the classic-control envs on the device (API level 6; must be
 * included by itself, mxv.h does not include it).
 * Part of the C ABI of libmxv.so (see mxv.h for the engine's handle, status codes and stream contract).
 *
 * A frame is the scene the reference's render() draws (cartpole.py:209-304, acrobot.py:279-367, mountain_car.py:169-274,
 * continuous_mountain_car.py:191-292) — the same primitives, integer coordinates, colours and draw order — rasterised by the engine's
 * own integer rule (4 x 4 samples per pixel, coverage blend, 1-px lines), flipped vertically: uint8 [H][W][3] RGB, row 0
 * at the top, the layout of the reference's np.transpose(pixels3d(screen), (1, 0, 2)).  CartPole / MountainCar*: 400 x 600,
 * Acrobot: 500 x 500.  Pendulum (its frame blits an image asset) and the toy_text engines have no frame: MXV_ERR_UNSUPPORTED. */
#ifndef MXV_RENDER_H
#define MXV_RENDER_H

#include "mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Scene records (mxv_render_scene_host): int32[MXV_RENDER_RECORD_INTS] = (op, 0xRRGGBB, n, r, x0, y0, x1, y1, x2, y2, x3, y3), the
 * n vertices in 1/8 px of the reference's surface (y up, before the flip); circles: the centre in (x0, y0), the radius r in px.
 * Float -> integer is int() (truncation toward zero) of the pixel value for gfxdraw / draw.line arguments and of 8 x the value for
 * the aalines points of MountainCar's track (one record per segment).  A primitive with a non-finite coordinate, or one beyond
 * +-2^20 px, is skipped: op MXV_RENDER_NONE (the reference raises there: int(nan)).  Every frame has MXV_RENDER_MAX_RECORDS slots;
 * those past the kind's draw list hold zeros. */
#define MXV_RENDER_RECORD_INTS 12
#define MXV_RENDER_MAX_RECORDS 112
enum {
    MXV_RENDER_NONE = 0,
    MXV_RENDER_AAPOLYGON = 1,
    MXV_RENDER_FILLED_POLYGON = 2,
    MXV_RENDER_AACIRCLE = 3,
    MXV_RENDER_FILLED_CIRCLE = 4,
    MXV_RENDER_HLINE = 5,
    MXV_RENDER_VLINE = 6,
    MXV_RENDER_LINE = 7,
    MXV_RENDER_AALINE = 8
};

/* Frame height and width of an env kind.  MXV_ERR_UNSUPPORTED for Pendulum, MXV_ERR_INVALID_ARG for an unknown kind or NULL outputs. */
int mxv_render_dims(int32_t env_id, int32_t *height, int32_t *width);

/* Renders `count` frames of the handle's current states into frames_dev (uint8 [count][H][W][3], device, 16-byte aligned): frame k
 * shows env indices_dev[k] (int32, device; repeats allowed), or env k when indices_dev is NULL (then count <= N).  Physics attributes
 * are the handle's, common or per-env (mxv_set_params_per_env).  Stream-ordered on the handle's stream, no synchronisation, recordable
 * into a caller's hipGraph (unless the state lives in an adopted observation buffer, mxv_adopt_obs).  An index outside [0, N) gives an
 * all-zero frame and an error (MXV_ERR_INVALID_ARG) that the next mxv_sync / *_host call reports.  Bad arguments (NULL handle or
 * frames, count <= 0, count > N without indices) return MXV_ERR_INVALID_ARG before the device is touched. */
int mxv_render(mxv_handle *h, const int32_t *indices_dev, int64_t count, uint8_t *frames_dev);

/* The same into host memory (uint8 [count][H][W][3]) with host indices (or NULL): synchronises, reports index errors itself. */
int mxv_render_host(mxv_handle *h, const int32_t *indices_host, int64_t count, uint8_t *frames_host);

/* The integer draw list the device computes for those frames: int32 [count][MXV_RENDER_MAX_RECORDS][MXV_RENDER_RECORD_INTS] into host
 * memory (see the record layout above).  Synchronises. */
int mxv_render_scene_host(mxv_handle *h, const int32_t *indices_host, int64_t count, int32_t *records_host);

#ifdef __cplusplus
}
#endif
#endif /* MXV_RENDER_H */
