/* mxv_render.h — OPTIONAL frame rendering: render_mode="rgb_array" of the classic-control envs on the device (API level 6; must be
 * included by itself, mxv.h does not include it).
 * Part of the C ABI of libmxv.so (see mxv.h for the engine's handle, status codes and stream contract).
 *
 * A frame is the scene the reference's render() draws (cartpole.py:209-304, acrobot.py:279-367, mountain_car.py:169-274,
 * continuous_mountain_car.py:191-292) — the same primitives, integer coordinates, colours and draw order — rasterised by the engine's
 * own integer rule (4 x 4 samples per pixel, coverage blend, 1-px lines), flipped vertically: uint8 [H][W][3] RGB, row 0
 * at the top, the layout of the reference's np.transpose(pixels3d(screen), (1, 0, 2)).  CartPole / MountainCar*: 400 x 600,
 * Acrobot: 500 x 500.  The toy_text engines have no frame: MXV_ERR_UNSUPPORTED.
 *
 * Pendulum-v1 (pendulum.py:167-261, 500 x 500) blits an image asset, the torque arrow (assets/clockwise.png), which the engine does not
 * carry: the caller supplies it (mxv_render_attach_image).  Until then every frame and pixel call on a Pendulum handle returns
 * MXV_ERR_UNSUPPORTED, and so does the handle-free mxv_render_dims(MXV_PENDULUM).  With an image attached the handle also tracks the
 * reference's render state `last_u` per env: NaN (= None) after a reset (mxv_reset, masked or not, mxv_reset_host, an autoreset inside a
 * step), else the float32 clip of the env's last action to [-max_torque, max_torque] (the step's own clip, pendulum.py:127-128); a NaN
 * action leaves NaN, and then no arrow is drawn (the reference raises there).  mxv_set_state leaves it unchanged.  The arrow is an
 * MXV_RENDER_BLIT record rasterised by the engine's own rule (below), not SDL's smoothscale / blend. */
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
    MXV_RENDER_AALINE = 8,
    /* (op, 0, 0, 0, x, y, w, h, flip_x, flip_y, 0, 0) in whole surface pixels (y before the final flip): surface pixel (px, py) with
     * 0 <= py - y < h, 0 <= px - x < w shows the scaled image's pixel (r, c) = (py - y, px - x), r -> h - 1 - r when flip_y and
     * c -> w - 1 - c when flip_x.  That pixel is the rounded mean (sum + n / 2) / n of each straight-RGBA channel over the n source
     * pixels of rows [floor(r Hs / h), ceil((r + 1) Hs / h)) and columns likewise (Hs x Ws the attached image), and it is blended as
     * d' = (s a + d (255 - a) + 127) / 255 per RGB channel, a its mean alpha.  w = 0 draws nothing. */
    MXV_RENDER_BLIT = 9
};

/* Frame height and width of an env kind.  MXV_ERR_UNSUPPORTED for Pendulum, MXV_ERR_INVALID_ARG for an unknown kind or NULL outputs. */
int mxv_render_dims(int32_t env_id, int32_t *height, int32_t *width);

/* Frame height and width of a handle: mxv_render_dims of its kind, and 500 x 500 for a Pendulum handle with an image attached
 * (MXV_ERR_UNSUPPORTED without one). */
int mxv_render_frame_dims(mxv_handle *h, int32_t *height, int32_t *width);

/* Pendulum handles only (MXV_ERR_UNSUPPORTED for any other kind): copies the arrow image, uint8 [height][width][4] straight RGBA in host
 * memory (1 <= height, width <= 1024), to the device and builds its summed-area table there; every env's last_u becomes NaN (None).
 * Calling it again replaces the image.  Synchronises the handle's stream; not recordable into a hipGraph. */
int mxv_render_attach_image(mxv_handle *h, const uint8_t *rgba_host, int32_t height, int32_t width);

/* last_u of every env, float32 [N] in host memory, NaN = None (checkpoints).  MXV_ERR_UNSUPPORTED without an attached image.  Both
 * synchronise the handle's stream. */
int mxv_render_get_torques_host(mxv_handle *h, float *last_u_host);
int mxv_render_set_torques_host(mxv_handle *h, const float *last_u_host);

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

/* -- pixel observations: the frame reduced to what a pixel learner reads (tests/pixels_host.py) ----------------------
 * A pixel observation of size height x width (1 <= height <= H, 1 <= width <= W) with `channels` 1 (gray) or 3 (RGB) is a function
 * of the frame above, computed without writing the frame anywhere:
 *   gray (first):  Y = (4899 R + 9617 G + 1868 B + 8192) >> 14 per source pixel (OpenCV's documented fixed-point BT.601 weights);
 *   area resize:   output pixel (i, j) is the rounded mean (sum + n / 2) / n, in integers, over the n source pixels of rows
 *                  [floor(i H / height), ceil((i + 1) H / height)) and columns [floor(j W / width), ceil((j + 1) W / width))
 *                  (torch.nn.functional.adaptive_avg_pool2d's windows; NOT OpenCV's INTER_AREA at non-integer ratios).
 * Layout uint8 [height][width] (gray) or [height][width][3], row 0 at the top.  The pipeline it replaces: the reference's
 * PixelObservationWrapper -> GrayScaleObservation -> ResizeObservation (pixel_observation.py:165-190, gray_scale_observation.py:50-64,
 * resize_observation.py:48-70).  Attributes, indices, errors and stream order are those of mxv_render.  Argument errors (height /
 * width out of range, channels not 1 or 3, copies < 1, NULL outputs, strides below one observation, a misaligned output or index
 * pointer of mxv_pixels) return MXV_ERR_INVALID_ARG, and Pendulum without an attached image MXV_ERR_UNSUPPORTED, before the device is
 * touched. */

/* Observations of `count` envs into out_dev (uint8 [count][height][width][channels], device, 16-byte aligned): observation k shows
 * env indices_dev[k] (int32, device; repeats allowed), or env k when indices_dev is NULL (then count <= N). */
int mxv_pixels(mxv_handle *h, const int32_t *indices_dev, int64_t count, int32_t height, int32_t width, int32_t channels,
               uint8_t *out_dev);

/* Observations of every env i whose mask_dev[i] is nonzero (uint8 [N], device; NULL = all envs) written `copies` times, to
 * out_dev + i * env_stride + c * copy_stride (bytes; c < copies): copies = 1 pushes a frame into one slot of a frame stack
 * (FrameStack, frame_stack.py:164-189), copies = num_stack fills the stack of a reset env.  16-byte stores wherever the
 * destination is 16-byte aligned, narrower stores elsewhere.  Workgroups of masked-out envs return after reading the mask. */
int mxv_pixels_strided(mxv_handle *h, const uint8_t *mask_dev, int32_t height, int32_t width, int32_t channels, int32_t copies,
                       uint8_t *out_dev, int64_t env_stride, int64_t copy_stride);

/* mxv_pixels into host memory with host indices (or NULL): synchronises, reports index errors itself. */
int mxv_pixels_host(mxv_handle *h, const int32_t *indices_host, int64_t count, int32_t height, int32_t width, int32_t channels,
                    uint8_t *out_host);

#ifdef __cplusplus
}
#endif
#endif /* MXV_RENDER_H */
