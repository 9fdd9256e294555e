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
};

// Makes the handle's device current and its state fp64-resident (mxv_adopt_obs), then fills *v.  MXV_ERR_* on failure (message set).
int render_view(mxv_handle *h, RenderView *v);
// The handle's env kind (no device work).
int32_t render_env_id(const mxv_handle *h);
// Records `message` as the handle's last error and returns `code`.
int render_fail(mxv_handle *h, int code, const char *message);

}  // namespace mxv
