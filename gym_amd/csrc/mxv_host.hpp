// mxv_host.hpp — host-side bookkeeping shared by the objects behind the C ABI (include/mxv.h).
//
// Error plumbing for all of them (mxv_handle, mxv_tab, mxv_bj, mxv_norm, mxv_subnorm, mxv_placed): fail() records the message on
// the object, or — for a NULL object, i.e. a failed create — in a per-thread slot of that object TYPE, which its *_last_error(NULL)
// reports.  HostCore: what the three engine handles (classic control, tabular, Blackjack) keep alike — device, stream, error word,
// step / reset counters and the device clock, seeds, episode statistics — and the calls that only touch it.  Each exported function
// stays a short forwarder in its family's file; a step only one family needs stays there too.  The handle-free policy calls have their
// own slots and argument checks in mxv_policy_host.hpp.  Host code only: no kernels here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <type_traits>

#include "../../include/mxv.h"

namespace mxv {

// one-thread kernels on `stream` (mxv_kernels.hip): *dst = value / *dst += delta (two's complement: a negative delta subtracts)
hipError_t launch_set_word(uint64_t *dst, uint64_t value, hipStream_t stream);
hipError_t launch_add_word(uint64_t *dst, uint64_t delta, hipStream_t stream);

template <class H>
std::string &create_error() {
    thread_local std::string s;
    return s;
}

template <class H>
int fail(H *h, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    (h ? h->error : create_error<H>()) = buf;
    return code;
}

template <class H>
const char *last_error(const H *h) {
    return h ? h->error.c_str() : create_error<H>().c_str();
}

// Caller-owned tensors on their element's natural boundary: an odd address would not fault on this device (unaligned global access is
// enabled) but tears every coalesced burst, and it is a caller bug either way — refused up front with the tensor's name
// (tests/c_consumer/abi_fuzz.c).
template <class H>
int check_aligned(H *h, const void *p, size_t bytes, const char *what) {
    if (p && ((uintptr_t)p & (bytes - 1)) != 0) return fail(h, MXV_ERR_INVALID_ARG, "%s pointer %p is not %zu-byte aligned", what, p, bytes);
    return MXV_OK;
}

}  // namespace mxv

#define MXV_HIP(h, expr)                                                                                   \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return ::mxv::fail((h), MXV_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// in a create function: a failed HIP call becomes the create error of h's type, and `destroy` tears down the half-built object
#define MXV_CREATE_HIP(h, destroy, expr)                                                                                  \
    do {                                                                                                                  \
        hipError_t e_ = (expr);                                                                                           \
        if (e_ != hipSuccess) {                                                                                           \
            ::mxv::fail<std::remove_pointer_t<decltype(h)>>(nullptr, MXV_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
            destroy(h);                                                                                                   \
            return MXV_ERR_HIP;                                                                                           \
        }                                                                                                                 \
    } while (0)

// every object type names its NULL message: static constexpr const char *kNullMessage
#define MXV_CHECK(h) \
    if (!(h)) return ::mxv::fail((h), MXV_ERR_INVALID_ARG, "%s", std::remove_pointer_t<decltype(h)>::kNullMessage)

namespace mxv {

struct HostCore {
    explicit HostCore(const char *api_prefix) : api(api_prefix) {}
    const char *api;                 // prefix of the family's entry points ("mxv", "mxv_tab", "mxv_bj"), for messages
    int device = 0;
    int64_t num_envs = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // Latched kernel error words: one block of pinned, coherent, device-mapped host memory (alloc_latch).  The kernels raise their
    // single-bit codes in it with plain stores; the host reads and clears it after a stream synchronisation — no copy command follows a
    // launch.  err[0]: the step / rollout kernels; err[kRenderLatchWord]: the render kernels (a plain store each, the host ORs them).
    int32_t *err = nullptr;          // the block as the kernels address it (stable for the handle's life: recorded hipGraphs keep it)
    volatile int32_t *err_host = nullptr;   // the same block as the host reads it
    std::string error;
    uint64_t t = 0;                  // vector steps taken (the action / step stream position)
    uint32_t r = 0;                  // explicit resets
    uint64_t *t_dev = nullptr;       // device clock: the step index in device memory (see mxv_set_device_clock)
    bool dev_clock = false;
    uint64_t base_seed = 0, action_seed = 0;
    uint64_t *seeds = nullptr;       // optional per-env seeds
    bool was_reset = false;
    // episode statistics (RecordEpisodeStatistics fused into the kernels): running returns, dense staging of host steps, the caller's
    // trajectory outputs
    float *ep_acc = nullptr, *st_ep_r = nullptr, *ep_return_out = nullptr;
    int32_t *st_ep_l = nullptr, *ep_length_out = nullptr;
};

constexpr int kLatchWords = 2, kRenderLatchWord = 1;
// the block is padded to one 64-byte line of its own: nothing else of the host shares the line the kernels store into over the bus
constexpr size_t kLatchBytes = 64;
static_assert(kLatchWords * sizeof(int32_t) <= kLatchBytes, "the latch words fit their line");

inline hipError_t alloc_latch(HostCore *h) {
    void *host = nullptr, *dev = nullptr;
    hipError_t e = hipHostMalloc(&host, kLatchBytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return e;
    h->err_host = (volatile int32_t *)host;
    for (int i = 0; i < kLatchWords; ++i) h->err_host[i] = 0;
    e = hipHostGetDevicePointer(&dev, host, 0);
    if (e == hipSuccess) h->err = (int32_t *)dev;
    return e;
}

inline int use_device(HostCore *h) {
    MXV_HIP(h, hipSetDevice(h->device));
    return MXV_OK;
}

// Device clock: the word follows the host counter through a one-thread kernel on the handle's stream — captured with the launches when a
// caller's hipGraph is being recorded.  `delta` < 0 takes a step back.
inline int clock_set(HostCore *h) {
    if (h->dev_clock) MXV_HIP(h, launch_set_word(h->t_dev, h->t, h->stream));
    return MXV_OK;
}
inline int clock_add(HostCore *h, int64_t delta) {
    h->t += (uint64_t)delta;
    if (h->dev_clock) MXV_HIP(h, launch_add_word(h->t_dev, (uint64_t)delta, h->stream));
    return MXV_OK;
}

inline int get_counters(HostCore *h, uint64_t *t, uint32_t *r) {
    if (h->dev_clock) {  // graphs the caller replays advance the device word only: read it (synchronises the handle's stream)
        if (int rc = use_device(h)) return rc;
        MXV_HIP(h, hipMemcpyAsync(&h->t, h->t_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        MXV_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (t) *t = h->t;
    if (r) *r = h->r;
    return MXV_OK;
}

inline int set_counters(HostCore *h, uint64_t t, uint32_t r) {
    h->t = t;
    h->r = r;
    if (!h->dev_clock) return MXV_OK;
    if (int rc = use_device(h)) return rc;
    return clock_set(h);
}

inline int set_device_clock(HostCore *h, int32_t on) {
    if (int rc = use_device(h)) return rc;
    if (on && !h->dev_clock) {
        MXV_HIP(h, launch_set_word(h->t_dev, h->t, h->stream));
        h->dev_clock = true;
    } else if (!on && h->dev_clock) {
        MXV_HIP(h, hipMemcpyAsync(&h->t, h->t_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        MXV_HIP(h, hipStreamSynchronize(h->stream));
        h->dev_clock = false;
    }
    return MXV_OK;
}

// The latched error words once the stream has drained: their OR, cleared (0 when nothing was latched).
inline int32_t take_latched_drained(HostCore *h) {
    int32_t word = 0;
    for (int i = 0; i < kLatchWords; ++i) {
        const int32_t w = h->err_host[i];
        if (w != 0) h->err_host[i] = 0;
        word |= w;
    }
    return word;
}

// The latched error word, read (synchronises the stream) and cleared: *word = 0 when nothing was latched.  What a raised bit means is
// the family's to say.
inline int take_latched(HostCore *h, int32_t *word) {
    *word = 0;
    MXV_HIP(h, hipStreamSynchronize(h->stream));
    *word = take_latched_drained(h);
    return MXV_OK;
}

// Drains the stream, then restarts the counters under a new base seed; per-env seeds replace it where given (stream-ordered upload).
inline int reseed(HostCore *h, uint64_t base_seed, const uint64_t *per_env_seeds_host) {
    if (int rc = use_device(h)) return rc;
    MXV_HIP(h, hipStreamSynchronize(h->stream));
    h->base_seed = base_seed;
    h->t = 0;
    h->r = 0;
    if (int rc = clock_set(h)) return rc;
    if (per_env_seeds_host) {
        const size_t bytes = (size_t)h->num_envs * sizeof(uint64_t);
        if (!h->seeds) MXV_HIP(h, hipMalloc((void **)&h->seeds, bytes));
        MXV_HIP(h, hipMemcpyAsync(h->seeds, per_env_seeds_host, bytes, hipMemcpyHostToDevice, h->stream));
        MXV_HIP(h, hipStreamSynchronize(h->stream));
    } else if (h->seeds) {
        MXV_HIP(h, hipStreamSynchronize(h->stream));
        MXV_HIP(h, hipFree(h->seeds));
        h->seeds = nullptr;
    }
    return MXV_OK;
}

// int32 [N] state and TimeLimit counters (tabular, Blackjack) to and from host arrays; either may be NULL.  Writing one stands in for reset().
inline int read_state32(HostCore *h, const int32_t *state, const int32_t *elapsed, int32_t *state_host, int32_t *elapsed_host) {
    if (int rc = use_device(h)) return rc;
    const size_t bytes = (size_t)h->num_envs * sizeof(int32_t);
    if (state_host) MXV_HIP(h, hipMemcpyAsync(state_host, state, bytes, hipMemcpyDeviceToHost, h->stream));
    if (elapsed_host) MXV_HIP(h, hipMemcpyAsync(elapsed_host, elapsed, bytes, hipMemcpyDeviceToHost, h->stream));
    MXV_HIP(h, hipStreamSynchronize(h->stream));
    return MXV_OK;
}
inline int write_state32(HostCore *h, int32_t *state, int32_t *elapsed, const int32_t *state_host, const int32_t *elapsed_host) {
    if (int rc = use_device(h)) return rc;
    const size_t bytes = (size_t)h->num_envs * sizeof(int32_t);
    if (state_host) MXV_HIP(h, hipMemcpyAsync(state, state_host, bytes, hipMemcpyHostToDevice, h->stream));
    if (elapsed_host) MXV_HIP(h, hipMemcpyAsync(elapsed, elapsed_host, bytes, hipMemcpyHostToDevice, h->stream));
    MXV_HIP(h, hipStreamSynchronize(h->stream));
    h->was_reset = true;
    return MXV_OK;
}

// ---- episode statistics (gym/wrappers/record_episode_statistics.py:96-151) ----
inline int episode_stats(HostCore *h, int32_t enable) {
    if (int rc = use_device(h)) return rc;
    MXV_HIP(h, hipStreamSynchronize(h->stream));
    const size_t n = (size_t)h->num_envs;
    if (enable && !h->ep_acc) {
        MXV_HIP(h, hipMalloc((void **)&h->ep_acc, n * sizeof(float)));
        MXV_HIP(h, hipMalloc((void **)&h->st_ep_r, n * sizeof(float)));
        MXV_HIP(h, hipMalloc((void **)&h->st_ep_l, n * sizeof(int32_t)));
        MXV_HIP(h, hipMemsetAsync(h->ep_acc, 0, n * sizeof(float), h->stream));
        MXV_HIP(h, hipMemsetAsync(h->st_ep_r, 0, n * sizeof(float), h->stream));
        MXV_HIP(h, hipMemsetAsync(h->st_ep_l, 0, n * sizeof(int32_t), h->stream));
        MXV_HIP(h, hipStreamSynchronize(h->stream));
    } else if (!enable && h->ep_acc) {
        MXV_HIP(h, hipFree(h->ep_acc));
        MXV_HIP(h, hipFree(h->st_ep_r));
        MXV_HIP(h, hipFree(h->st_ep_l));
        h->ep_acc = h->st_ep_r = nullptr;
        h->st_ep_l = nullptr;
    }
    return MXV_OK;
}

inline int set_episode_outputs(HostCore *h, float *ep_return_dev, int32_t *ep_length_dev) {
    if (int rc = use_device(h)) return rc;
    MXV_HIP(h, hipStreamSynchronize(h->stream));
    h->ep_return_out = ep_return_dev;
    h->ep_length_out = ep_length_dev;
    return MXV_OK;
}

inline int episode_stats_host(HostCore *h, float *ep_return_host, int32_t *ep_length_host, float *running_return_host) {
    if (!h->ep_acc) return fail(h, MXV_ERR_INVALID_ARG, "episode statistics are not enabled (%s_episode_stats)", h->api);
    if (int rc = use_device(h)) return rc;
    const size_t n = (size_t)h->num_envs;
    if (ep_return_host) MXV_HIP(h, hipMemcpyAsync(ep_return_host, h->st_ep_r, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (ep_length_host) MXV_HIP(h, hipMemcpyAsync(ep_length_host, h->st_ep_l, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (running_return_host) MXV_HIP(h, hipMemcpyAsync(running_return_host, h->ep_acc, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    MXV_HIP(h, hipStreamSynchronize(h->stream));
    return MXV_OK;
}

inline int set_running_returns(HostCore *h, const float *running_return_host) {
    if (!h->ep_acc) return fail(h, MXV_ERR_INVALID_ARG, "episode statistics are not enabled (%s_episode_stats)", h->api);
    if (!running_return_host) return fail(h, MXV_ERR_INVALID_ARG, "running_return pointer is NULL");
    if (int rc = use_device(h)) return rc;
    MXV_HIP(h, hipMemcpyAsync(h->ep_acc, running_return_host, (size_t)h->num_envs * sizeof(float), hipMemcpyHostToDevice, h->stream));
    MXV_HIP(h, hipStreamSynchronize(h->stream));
    return MXV_OK;
}

// ---- stream, teardown ----
inline int set_stream(HostCore *h, void *stream) {
    if (int rc = use_device(h)) return rc;
    if (h->stream) MXV_HIP(h, hipStreamSynchronize(h->stream));
    if (h->own_stream && h->stream) MXV_HIP(h, hipStreamDestroy(h->stream));
    h->stream = (hipStream_t)stream;
    h->own_stream = false;
    return MXV_OK;
}

// The common part of *_destroy, in two halves around the family's own teardown: drain() first, then free_core() with the family's
// device buffers (NULL entries are skipped) — it destroys an owned stream last.
inline void drain(HostCore *h) {
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
}
inline void free_core(HostCore *h, std::initializer_list<void *> family_buffers) {
    if (h->err_host) (void)hipHostFree((void *)h->err_host);
    for (void *p : {(void *)h->t_dev, (void *)h->seeds, (void *)h->ep_acc, (void *)h->st_ep_r, (void *)h->st_ep_l})
        if (p) (void)hipFree(p);
    for (void *p : family_buffers)
        if (p) (void)hipFree(p);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
}

}  // namespace mxv
