// primitives.hip — the device math helpers of gym_amd/csrc/mxv_device.hpp and mxv_divide.hpp, as shipped, one element-wise kernel per
// helper and per template instantiation the engine uses.  Nothing here restates a helper: every op below calls the header's function.
// tests/test_gpu_device_math.py builds this file with the library's flags and drives it through ctypes; tests/test_kernel_resources.py
// cross-compiles it on the CPU.
//
// Host entry points: extern "C" hipError_t <op>(const T *a, const T *b, const T *c, T *o, T *p, int64_t n) with T = double or float
// (host arrays; a null input reads as 0, a null output is not copied back).  Each call allocates, copies in, launches, synchronises,
// copies out and frees on the null stream, and returns the first HIP error.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../gym_amd/csrc/mxv_device.hpp"

using namespace mxv;

namespace {

template <typename T, typename Op>
__global__ void elementwise(const T *a, const T *b, const T *c, T *o, T *p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    T ro = 0, rp = 0;
    Op::apply(a[i], b[i], c[i], ro, rp);
    o[i] = ro;
    p[i] = rp;
}

#define MXV_CHECK(x)                        \
    do {                                    \
        const hipError_t e_ = (x);          \
        if (e_ != hipSuccess && err == hipSuccess) err = e_; \
    } while (0)

template <typename T, typename Op>
hipError_t run(const T *a, const T *b, const T *c, T *o, T *p, int64_t n) {
    if (n <= 0) return hipSuccess;
    hipError_t err = hipSuccess;
    const size_t bytes = (size_t)n * sizeof(T);
    T *d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const T *in[3] = {a, b, c};
    for (int k = 0; k < 5 && err == hipSuccess; ++k) MXV_CHECK(hipMalloc((void **)&d[k], bytes));
    for (int k = 0; k < 3 && err == hipSuccess; ++k)
        MXV_CHECK(in[k] ? hipMemcpy(d[k], in[k], bytes, hipMemcpyHostToDevice) : hipMemset(d[k], 0, bytes));
    if (err == hipSuccess) {
        const int threads = 256;
        hipLaunchKernelGGL((elementwise<T, Op>), dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, 0, d[0], d[1], d[2], d[3],
                           d[4], n);
        MXV_CHECK(hipGetLastError());
        MXV_CHECK(hipDeviceSynchronize());
    }
    if (o && err == hipSuccess) MXV_CHECK(hipMemcpy(o, d[3], bytes, hipMemcpyDeviceToHost));
    if (p && err == hipSuccess) MXV_CHECK(hipMemcpy(p, d[4], bytes, hipMemcpyDeviceToHost));
    for (int k = 0; k < 5; ++k)
        if (d[k]) MXV_CHECK(hipFree(d[k]));
    return err;
}

}  // namespace

#define MXV_OP(name, T, ...)                                                                                   \
    namespace {                                                                                                \
    struct name##_op {                                                                                         \
        __device__ __forceinline__ static void apply(T a, T b, T c, T &o, T &p) { __VA_ARGS__; }                    \
    };                                                                                                         \
    }                                                                                                          \
    extern "C" hipError_t name(const T *a, const T *b, const T *c, T *o, T *p, int64_t n) {                    \
        return run<T, name##_op>(a, b, c, o, p, n);                                                            \
    }

// ---- sin / cos: o = sin(a), p = cos(a) -----------------------------------------------------------------------------------------------
MXV_OP(sincos_kernel_f0, double, sincos_kernel<0>(a, &o, &p))
MXV_OP(sincos_kernel_f1, double, sincos_kernel<1>(a, &o, &p))
MXV_OP(sincos_medium_f0, double, sincos_medium<0>(a, &o, &p))
MXV_OP(sincos_medium_f1, double, sincos_medium<1>(a, &o, &p))
MXV_OP(sincos_medium_f2, double, sincos_medium<2>(a, &o, &p))
MXV_OP(sincos_medium_f3, double, sincos_medium<3>(a, &o, &p))
// F3 of every env kind: fma3_for<MXV_CARTPOLE>() = fma3_for<MXV_MOUNTAINCAR>() = 0, MountainCarContinuous 1, Acrobot 2, Pendulum 3
// (and Pendulum's two-envs-per-lane form, 3 & ~1 = 2)
MXV_OP(mx_sincos_guarded_cartpole, double, mx_sincos<true, fma3_for<MXV_CARTPOLE>()>(a, &o, &p))
MXV_OP(mx_sincos_guarded_mcc, double, mx_sincos<true, fma3_for<MXV_MOUNTAINCAR_CONT>()>(a, &o, &p))
MXV_OP(mx_sincos_guarded_acrobot, double, mx_sincos<true, fma3_for<MXV_ACROBOT>()>(a, &o, &p))
MXV_OP(mx_sincos_guarded_pendulum, double, mx_sincos<true, fma3_for<MXV_PENDULUM>()>(a, &o, &p))
MXV_OP(mx_sincos_fast_cartpole, double, mx_sincos<false, fma3_for<MXV_CARTPOLE>()>(a, &o, &p))
MXV_OP(mx_sincos_fast_mcc, double, mx_sincos<false, fma3_for<MXV_MOUNTAINCAR_CONT>()>(a, &o, &p))
MXV_OP(mx_sincos_fast_acrobot, double, mx_sincos<false, fma3_for<MXV_ACROBOT>()>(a, &o, &p))
MXV_OP(mx_sincos_fast_pendulum, double, mx_sincos<false, fma3_for<MXV_PENDULUM>()>(a, &o, &p))
MXV_OP(sincos_small_or_general_op, double, sincos_small_or_general(a, &o, &p))

// ---- division: o = a / b (b = CartPole's total_mass literal for div_par) ----------------------------------------------------------
MXV_OP(div_par_finite, double, o = (div_par<PM_DEFAULT, true>(a, 0.1 + 1.0)))
MXV_OP(div_par_fixup, double, o = (div_par<PM_DEFAULT, false>(a, 0.1 + 1.0)))
MXV_OP(div_with_rcp_op, double, o = div_with_rcp(a, b, refined_rcp(b)))
MXV_OP(div_shared_op, double, o = div_shared(a, b, refined_rcp(b)))
// p = plain_operand(a) | plain_divisor(a) << 1 | plain_delta(a) << 2
MXV_OP(plain_guards, double, p = (double)((plain_operand(a) ? 1 : 0) | (plain_divisor(a) ? 2 : 0) | (plain_delta(a) ? 4 : 0)))

// ---- remainders by 2 pi (Pendulum's angle_normalize) ---------------------------------------------------------------------------------
MXV_OP(fmod_const_2pi, double, o = fmod_const(a, 2 * kPi, 1.0 / (2 * kPi)))
MXV_OP(np_remainder_2pi, double, o = np_remainder(a, 2 * kPi))
MXV_OP(np_remainder_bounded_2pi, double, o = np_remainder_bounded(a, 2 * kPi))

// ---- clamps: o = clamp(a, lo = b, hi = c) --------------------------------------------------------------------------------------------
MXV_OP(clamp_range_f64, double, o = clamp_range(a, b, c))
MXV_OP(clamp_range_hi_first_f64, double, o = clamp_range_hi_first(a, b, c))
MXV_OP(clamp_range_f32, float, o = clamp_range(a, b, c))
MXV_OP(clamp_range_hi_first_f32, float, o = clamp_range_hi_first(a, b, c))
MXV_OP(nan_through_op, double, o = nan_through(a, b))

// ---- Pendulum's glibc powf(u, 2.0f) restatement --------------------------------------------------------------------------------------
MXV_OP(glibc_powf_square_op, float, o = glibc_powf_square(a))
