/* The argument checks of mxv_squashed_sample and mxv_squashed_sample_backward (include/mxv_squashed.h) driven from plain C: every call
 * below must be refused with MXV_ERR_INVALID_ARG and a message in the header's own slot, mxv_squashed_last_error, before the device is
 * touched (the device addresses are invented and never dereferenced; scale and bias are real host arrays, which the checks read).
 * Built by tests/test_squashed_args_sanitized.py with AddressSanitizer + UBSan against the sanitized library, so the host validation —
 * the reads of scale and bias, the range arithmetic at the 2^40 bound and at the top of the address space, the alignment loop, the
 * thread-local error slot — runs instrumented. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "mxv_policy.h"
#include "mxv_squashed.h"

#define P(x) ((void *)(uintptr_t)(x))
#define M 0x100000ull
static int calls = 0, bad = 0;
static const char *api = "mxv_squashed_sample:";

static void expect(int rc, const char *what) {
    const char *msg = mxv_squashed_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what) || strstr(msg, api) != msg) {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s' from %s\n", rc, msg ? msg : "(null)", what, api);
    }
}

static const float *g_scale = NULL, *g_bias = NULL;

/* mean M, log_std 2M, actions 3M, log_prob 4M, counter 6M, step_used 7M */
static int draw(int64_t N, int32_t D, void *mean, int64_t mld, void *ls, int64_t sld, void *step_dev, void *used, void *act, int64_t ald, void *lp) {
    return mxv_squashed_sample(NULL, N, D, (const float *)mean, mld, (const float *)ls, sld, g_scale, g_bias, 1u, 2u, 3u, (uint64_t *)step_dev,
                               (uint64_t *)used, (float *)act, ald, (float *)lp);
}

/* mean M, log_std 2M, grad_actions 3M, grad_log_prob 4M, grad_mean 5M, grad_log_std 8M, counter 6M */
static int back(int64_t N, int32_t D, void *mean, int64_t mld, void *ls, int64_t sld, void *step_dev, void *ga, int64_t gald, void *glp, void *gm,
                int64_t gmld, void *gs, int64_t gsld) {
    return mxv_squashed_sample_backward(NULL, N, D, (const float *)mean, mld, (const float *)ls, sld, g_scale, g_bias, 1u, 2u, 3u,
                                        (const uint64_t *)step_dev, (const float *)ga, gald, (const float *)glp, (float *)gm, gmld, (float *)gs, gsld);
}

int main(void) {
    const int64_t big = (int64_t)1 << 62;
    float scale[4] = {2.0f, 1.0f, 0.5f, 64.0f}, bias[4] = {0.0f, -1.0f, 3.0f, 100.0f};
    g_scale = scale;
    g_bias = bias;
    expect(draw(16, 3, NULL, 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "mean pointer is NULL");
    expect(draw(16, 3, P(M), 3, NULL, 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "log_std pointer is NULL");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, NULL, 3, P(4 * M)), "actions pointer is NULL");
    expect(draw(0, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "N =");
    expect(draw(INT64_MIN, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "N =");
    expect(draw(16, 0, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "D =");
    expect(draw(16, 5, P(M), 5, P(2 * M), 5, NULL, NULL, P(3 * M), 5, P(4 * M)), "D =");
    expect(draw(16, INT32_MIN, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "D =");
    expect(draw(16, 3, P(M), 2, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "mean_ld =");
    expect(draw(16, 3, P(M), -5, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "mean_ld =");
    expect(draw(16, 3, P(M), 3, P(2 * M), 2, NULL, NULL, P(3 * M), 3, P(4 * M)), "log_std_ld =");
    expect(draw(16, 3, P(M), 3, P(2 * M), -1, NULL, NULL, P(3 * M), 3, P(4 * M)), "log_std_ld =");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 2, P(4 * M)), "actions_ld =");
    expect(draw(16, 3, P(M), 3, P(2 * M), 0, NULL, NULL, P(3 * M), 0, P(4 * M)), "actions_ld =");
    expect(draw(16, 3, P(M), big, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "2^40");
    expect(draw(16, 3, P(M), 3, P(2 * M), big, NULL, NULL, P(3 * M), 3, P(4 * M)), "2^40");
    expect(draw(16, 3, P(M), 3, P(2 * M), 0, NULL, NULL, P(3 * M), INT64_MAX, P(4 * M)), "2^40");
    expect(draw(big, 3, P(M), INT64_MAX, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "2^40");
    expect(draw(((int64_t)1 << 40) / 3 + 1, 3, P(M), 3, P(2 * M), 0, NULL, NULL, P(3 * M), 3, P(4 * M)), "2^40");
    /* the action space: scale in [2^-33, 64] and finite, bias finite; only the first D entries count */
    scale[1] = 0.0f;
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "scale[1] =");
    scale[1] = -1.0f;
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "scale[1] =");
    scale[1] = 1.0f;
    scale[2] = 64.5f;
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "scale[2] =");
    scale[2] = 0x1p-34f;
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "scale[2] =");
    scale[2] = NAN;
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "scale[2] =");
    scale[2] = 0.5f;
    scale[0] = INFINITY;
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "scale[0] =");
    scale[0] = 2.0f;
    bias[2] = INFINITY;
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "bias[2] =");
    bias[2] = NAN;
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "bias[2] =");
    bias[2] = 3.0f;
    scale[3] = NAN;      /* beyond D = 3: not read as part of the action space; the call fails on what comes next */
    bias[3] = NAN;
    expect(draw(16, 3, P(M + 2), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "mean pointer");
    scale[3] = 64.0f;
    bias[3] = 100.0f;
    g_scale = NULL;      /* NULL: 1 and 0 */
    g_bias = NULL;
    /* pointers off their element's boundary */
    expect(draw(16, 3, P(M), 3, P(2 * M + 1), 0, NULL, NULL, P(3 * M), 3, P(4 * M)), "log_std pointer");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, P(6 * M + 4), NULL, P(3 * M), 3, P(4 * M)), "step_dev pointer");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(7 * M + 4), P(3 * M), 3, P(4 * M)), "step_used pointer");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M + 2), 3, P(4 * M)), "actions pointer");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M + 1)), "log_prob pointer");
    g_scale = scale;
    g_bias = bias;
    /* ranges that would wrap past the top of the address space */
    expect(draw(16, 3, P(UINTPTR_MAX - 7), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(4 * M)), "address space");
    expect(draw(16, 3, P(M), 3, P(UINTPTR_MAX - 7), 0, NULL, NULL, P(3 * M), 3, P(4 * M)), "address space");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(UINTPTR_MAX - 15), 3, P(4 * M)), "address space");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(UINTPTR_MAX - 3)), "address space");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, P(UINTPTR_MAX - 7), NULL, P(3 * M), 3, NULL), "address space");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(UINTPTR_MAX - 7), P(3 * M), 3, NULL), "address space");
    /* an output that shares a byte with an input or with another output */
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(M + 188), 3, P(4 * M)), "actions overlaps the mean");
    expect(draw(16, 3, P(M), 8, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(M + 4 * 122)), "log_prob overlaps the mean");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(M + 184), P(3 * M), 3, P(4 * M)), "step_used overlaps the mean");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(2 * M - 188), 3, P(4 * M)), "actions overlaps the log_std");
    expect(draw(16, 3, P(M), 3, P(2 * M), 0, NULL, NULL, P(3 * M), 3, P(2 * M + 8)), "log_prob overlaps the log_std");
    expect(draw(16, 3, P(M), 3, P(2 * M), 0, NULL, P(2 * M + 8), P(3 * M), 3, P(4 * M)), "step_used overlaps the log_std");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, P(3 * M + 184), NULL, P(3 * M), 3, P(4 * M)), "actions overlaps step_dev");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, P(4 * M), NULL, P(3 * M), 3, P(4 * M + 4)), "log_prob overlaps step_dev");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, P(6 * M), P(6 * M), P(3 * M), 3, P(4 * M)), "step_used overlaps step_dev");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, P(3 * M), 3, P(3 * M + 188)), "outputs actions and log_prob overlap");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M + 184), P(3 * M), 3, P(4 * M)), "outputs actions and step_used overlap");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(4 * M + 56), P(3 * M), 3, P(4 * M)), "outputs log_prob and step_used overlap");

    api = "mxv_squashed_sample_backward:";
    expect(back(16, 3, NULL, 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(8 * M), 3), "mean pointer is NULL");
    expect(back(16, 3, P(M), 3, NULL, 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(8 * M), 3), "log_std pointer is NULL");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), NULL, 3, NULL, 3), "both NULL");
    expect(back(-1, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(8 * M), 3), "N =");
    expect(back(16, 5, P(M), 5, P(2 * M), 5, NULL, P(3 * M), 5, P(4 * M), P(5 * M), 5, P(8 * M), 5), "D =");
    expect(back(16, 3, P(M), 2, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(8 * M), 3), "mean_ld =");
    expect(back(16, 3, P(M), 3, P(2 * M), 1, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(8 * M), 3), "log_std_ld =");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 2, P(4 * M), P(5 * M), 3, P(8 * M), 3), "grad_actions_ld =");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 0, P(8 * M), 3), "grad_mean_ld =");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(8 * M), 2), "grad_log_std_ld =");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), big, P(4 * M), P(5 * M), 3, P(8 * M), 3), "2^40");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), big, P(8 * M), 3), "2^40");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(8 * M), INT64_MAX), "2^40");
    scale[0] = 65.0f;
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(8 * M), 3), "scale[0] =");
    scale[0] = 2.0f;
    bias[1] = -INFINITY;
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(8 * M), 3), "bias[1] =");
    bias[1] = -1.0f;
    expect(back(16, 3, P(M), 3, P(2 * M), 3, P(6 * M + 4), P(3 * M), 3, P(4 * M), P(5 * M), 3, P(8 * M), 3), "step_dev pointer");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M + 2), 3, P(4 * M), P(5 * M), 3, P(8 * M), 3), "grad_actions pointer");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M + 1), P(5 * M), 3, P(8 * M), 3), "grad_log_prob pointer");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M + 2), 3, P(8 * M), 3), "grad_mean pointer");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(8 * M + 3), 3), "grad_log_std pointer");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(UINTPTR_MAX - 15), 3, P(4 * M), P(5 * M), 3, P(8 * M), 3), "address space");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, 0, P(UINTPTR_MAX - 3), P(5 * M), 3, P(8 * M), 3), "address space");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(UINTPTR_MAX - 15), 3, NULL, 0), "address space");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), NULL, 0, P(UINTPTR_MAX - 15), 3), "address space");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(M + 188), 3, P(8 * M), 3), "grad_mean overlaps the mean");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(2 * M - 188), 3), "grad_log_std overlaps the log_std");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, P(5 * M + 184), P(3 * M), 3, P(4 * M), P(5 * M), 3, P(8 * M), 3), "grad_mean overlaps step_dev");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(3 * M + 188), 3, P(8 * M), 3), "grad_mean overlaps the grad_actions");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(4 * M + 60), 3), "grad_log_std overlaps the grad_log_prob");
    expect(back(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M), 3, P(5 * M + 188), 3), "outputs grad_mean and grad_log_std overlap");
    /* the slot is this header's own: a refusal of the Gaussian sampler's call does not replace the message above */
    ++calls;
    if (mxv_policy_sample_gaussian(NULL, 0, 3, (const float *)P(M), 3, (const float *)P(2 * M), 3, 1u, 2u, 3u, NULL, (float *)P(3 * M), 3, NULL,
                                   NULL) != MXV_ERR_INVALID_ARG ||
        !strstr(mxv_policy_last_error(), "mxv_policy_sample_gaussian") || !strstr(mxv_squashed_last_error(), "outputs grad_mean and grad_log_std overlap")) {
        ++bad;
        printf("BAD: the slots are not separate: '%s' / '%s'\n", mxv_policy_last_error(), mxv_squashed_last_error());
    }
    printf("squashed_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
