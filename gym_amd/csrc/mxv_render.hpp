// mxv_render.hpp — what the frame renderer (mxv_render.hip) reads of a handle; the handle's layout stays private to mxv_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mxv.h"

namespace mxv {

// error-word bit a render launch latches for an env index outside [0, N) (mxv_sync reports it)
constexpr int32_t kRenderIndexErrorBit = 0x100;

struct RenderView {
    int32_t env_id;
    int64_t n;
    hipStream_t stream;
    const double *state;      // [S][N] fp64
    const double *params_pe;  // [MXV_MAX_PARAMS][N] or nullptr (then P)
    double P[MXV_MAX_PARAMS];
    int32_t *err;             // latched error word
    // Pendulum with an attached arrow image (mxv_render_attach_image); nullptr / 0 otherwise
    const float *last_u;      // [N] the reference's last_u, NaN = None
    const uint4 *sat;         // [img_h + 1][img_w + 1] summed-area table of the straight RGBA image
    int32_t img_h, img_w;
};

// Makes the handle's device current and its state fp64-resident (mxv_adopt_obs), then fills *v.  MXV_ERR_* on failure (message set).
int render_view(mxv_handle *h, RenderView *v);
// The handle's env kind (no device work).
int32_t render_env_id(const mxv_handle *h);
// Whether the handle has frames: a kind with a frame, or Pendulum with an attached image (no device work).
bool render_ready(const mxv_handle *h);
// Records `message` as the handle's last error and returns `code`.
int render_fail(mxv_handle *h, int code, const char *message);

// -- Pendulum's arrow (mxv_render.hip; called by mxv_api.cpp on the handle's stream) ----------------------------------------------------
// The summed-area table of a uint8 [h][w][4] device image into sat[h + 1][w + 1] (one workgroup).
hipError_t launch_blit_table(const uint8_t *rgba, uint4 *sat, int32_t h, int32_t w, hipStream_t stream);
// last_u after a reset: NaN where mask[i] != 0 (every env when mask is nullptr).
hipError_t launch_track_reset(float *last_u, const uint8_t *mask, int64_t n, hipStream_t stream);
// last_u after a step: the float32 clip of actions[i] to [-max_torque, max_torque] (params_pe row 1 when per-env), NaN where the step
// autoreset the env (its elapsed counter is 0 afterwards).
hipError_t launch_track_step(float *last_u, const float *actions, const void *elapsed, int32_t elapsed16, const double *params_pe,
                             double max_torque, int64_t n, hipStream_t stream);

}  // namespace mxv
