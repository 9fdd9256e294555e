// mxv_policy_host.hpp — the host side that the handle-free policy calls share (include/mxv_policy.h, include/mxv_policy_eval.h): their
// error slots, the argument checks that run before the device is touched, and the launch.  mxv_policy.hip, mxv_gaussian.hip and
// mxv_policy_eval.hip keep only what is their own: the ranges of their arguments, filling the kernel's struct and choosing the
// instantiation.  mxv_ppo.hip (include/mxv_ppo.h), mxv_vtrace.hip (include/mxv_vtrace.h) and mxv_gae.hip (include/mxv_gae.h) use the
// same Call with their own slots.
// Host code only: no kernels here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "mxv_host.hpp"
#include "mxv_policy_rule.hpp"

namespace mxv {

// The per-thread error slots of the handle-free calls (mxv::create_error).  The types have external linkage, so fail<PolicyCall>(nullptr, ...)
// in mxv_policy.hip and in mxv_gaussian.hip write the one string that mxv_policy_last_error reports (tests/c_consumer/gaussian_args.c).
struct PolicyCall {   // include/mxv_policy.h
    std::string error;
};
struct EvalCall {   // include/mxv_policy_eval.h: mxv_policy_eval_last_error
    std::string error;
};
struct PpoCall {   // include/mxv_ppo.h: mxv_ppo_last_error
    std::string error;
};
struct VtraceCall {   // include/mxv_vtrace.h: mxv_vtrace_last_error
    std::string error;
};
struct GaeCall {   // include/mxv_gae.h: mxv_gae_last_error, of mxv_gae and mxv_discounted_returns
    std::string error;
};
struct DqnCall {   // include/mxv_dqn.h: mxv_dqn_last_error
    std::string error;
};
struct ReplayCall {   // include/mxv_replay.h: mxv_replay_last_error
    std::string error;
};
struct PrioCall {   // include/mxv_prio.h: mxv_prio_last_error
    std::string error;
};
struct C51Call {   // include/mxv_c51.h: mxv_c51_last_error
    std::string error;
};
struct NStepCall {   // include/mxv_nstep.h: mxv_nstep_last_error
    std::string error;
};
struct QrCall {   // include/mxv_qr.h: mxv_qr_last_error
    std::string error;
};
struct TargetsCall {   // include/mxv_targets.h: mxv_targets_last_error
    std::string error;
};
struct SacCall {   // include/mxv_sac.h: mxv_sac_last_error
    std::string error;
};

namespace policy_host {

struct Range {   // the bytes [lo, lo + bytes) of one argument, of elements of `elem` bytes; lo == 0: absent
    const char *name;
    uintptr_t lo;
    uint64_t bytes, elem;
    const char *the = "the ";   // "output X overlaps the logits", but "... overlaps step_dev"
};
inline bool meet(const Range &a, const Range &b) { return a.lo && b.lo && a.lo < b.lo + b.bytes && b.lo < a.lo + a.bytes; }

// n rows of W floats, `ld` floats apart (ld == 0: one shared row)
inline uint64_t rows_bytes(int64_t n, int64_t ld, int32_t W) { return ((uint64_t)(n - 1) * (uint64_t)ld + (uint64_t)W) * 4; }

inline dim3 grid_of(int64_t tiles) { return dim3((unsigned)(tiles < rule::kMaxBlocks ? tiles : rule::kMaxBlocks)); }

// One entry point's checks and launch: messages start with its name, call its row count `count` ('N' envs for a sampler, 'M' rows for
// an evaluator) and go to the error slot `Slot`.  Every check returns MXV_OK or the recorded error's code.
template <class Slot>
struct Call {
    const char *api;
    char count;

    template <typename... T>
    int bad(const char *fmt, T... args) const {
        return fail<Slot>(nullptr, MXV_ERR_INVALID_ARG, fmt, args...);
    }

    // alignment and address-space fit of every range; then no output may share a byte with an input or with another output
    int check_ranges(int64_t n, const Range *ins, int n_in, const Range *outs, int n_out) const {
        for (int pass = 0; pass < 2; ++pass) {
            const Range *r = pass ? outs : ins;
            for (int i = 0; i < (pass ? n_out : n_in); ++i) {
                if (r[i].lo & (r[i].elem - 1))
                    return bad("%s: %s pointer %p is not %llu-byte aligned", api, r[i].name, (void *)r[i].lo, (unsigned long long)r[i].elem);
                if (r[i].lo && r[i].bytes > UINTPTR_MAX - r[i].lo)
                    return bad("%s: %s at %p with %c = %lld does not fit the address space", api, r[i].name, (void *)r[i].lo, count, (long long)n);
            }
        }
        for (int i = 0; i < n_out; ++i) {
            for (int j = 0; j < n_in; ++j)
                if (meet(outs[i], ins[j])) return bad("%s: output %s overlaps %s%s", api, outs[i].name, ins[j].the, ins[j].name);
            for (int j = i + 1; j < n_out; ++j)
                if (meet(outs[i], outs[j])) return bad("%s: outputs %s and %s overlap", api, outs[i].name, outs[j].name);
        }
        return MXV_OK;
    }

    int check_stride(int64_t ld, int64_t n) const {   // the 2^40 bound on what a row index reaches
        if (ld > rule::kMaxElems / n) return bad("%s: %c * ld = %lld * %lld is beyond 2^40 elements", api, count, (long long)n, (long long)ld);
        return MXV_OK;
    }

    // a categorical head: n rows of A logits and an action each
    int check_cat(int64_t n, int32_t A, const float *logits, int64_t ld, const void *actions) const {
        if (!logits) return bad("%s: logits pointer is NULL", api);
        if (!actions) return bad("%s: actions pointer is NULL", api);
        if (n < 1) return bad("%s: %c = %lld must be at least 1", api, count, (long long)n);
        if (A < 1 || A > rule::kMaxActions) return bad("%s: A = %d must be in 1..%d", api, (int)A, rule::kMaxActions);
        if (ld < A) return bad("%s: row stride ld = %lld must be at least A = %d", api, (long long)ld, (int)A);
        return check_stride(ld, n);
    }

    // a diagonal-Gaussian head: n rows of D means, log_stds (or one shared row) and actions
    int check_gauss(int64_t n, int32_t D, const float *mean, int64_t mean_ld, const float *log_std, int64_t log_std_ld, const float *actions,
                    int64_t actions_ld) const {
        if (!mean) return bad("%s: mean pointer is NULL", api);
        if (!log_std) return bad("%s: log_std pointer is NULL", api);
        if (!actions) return bad("%s: actions pointer is NULL", api);
        if (n < 1) return bad("%s: %c = %lld must be at least 1", api, count, (long long)n);
        if (D < 1 || D > rule::kMaxDim) return bad("%s: D = %d must be in 1..%d", api, (int)D, rule::kMaxDim);
        if (mean_ld < D) return bad("%s: row stride mean_ld = %lld must be at least D = %d", api, (long long)mean_ld, (int)D);
        if (log_std_ld != 0 && log_std_ld < D)
            return bad("%s: row stride log_std_ld = %lld must be 0 (one shared row) or at least D = %d", api, (long long)log_std_ld, (int)D);
        if (actions_ld < D) return bad("%s: row stride actions_ld = %lld must be at least D = %d", api, (long long)actions_ld, (int)D);
        for (const int64_t ld : {mean_ld, log_std_ld, actions_ld})
            if (int rc = check_stride(ld, n)) return rc;
        return MXV_OK;
    }

    int hip_failed(const char *what, hipError_t e) const { return fail<Slot>(nullptr, MXV_ERR_HIP, "%s: %s: %s", api, what, hipGetErrorString(e)); }

    // `kernel`(a) on `stream`: the grid of a.tiles tiles
    template <typename Args>
    int launch(const void *kernel, Args &a, void *stream) const {
        void *args[] = {&a};
        // hipLaunchKernel returns THIS launch's status (hipGetLastError would also report, and clear, an earlier call's error)
        const hipError_t e = hipLaunchKernel(kernel, grid_of(a.tiles), dim3(rule::kThreads), args, 0, (hipStream_t)stream);
        return e == hipSuccess ? MXV_OK : hip_failed("kernel launch", e);
    }

    // `kernel`(a) on `stream` with one workgroup per leaf, or per group of a level, of a sum tree (mxv_sum_tree.hpp, whose run_tree
    // launches the levels through this): `blocks` workgroups, no striding
    template <typename Args>
    int launch_blocks(const void *kernel, Args &a, int64_t blocks, void *stream) const {
        void *args[] = {&a};
        const hipError_t e = hipLaunchKernel(kernel, dim3((unsigned)blocks), dim3(rule::kThreads), args, 0, (hipStream_t)stream);
        return e == hipSuccess ? MXV_OK : hip_failed("kernel launch", e);
    }

    // a sampler's device step counter, advanced by one behind the draw; NULL: there is none
    int advance(uint64_t *step_dev, void *stream) const {
        if (!step_dev) return MXV_OK;
        const hipError_t e = launch_add_word(step_dev, 1, (hipStream_t)stream);
        return e == hipSuccess ? MXV_OK : hip_failed("step counter launch", e);
    }
};

}  // namespace policy_host
}  // namespace mxv
