/* The argument checks of the four calls of include/mxv_policy_eval.h driven from plain C: every call below must be refused with
 * MXV_ERR_INVALID_ARG and a message that names the call — in the header's own error slot, mxv_policy_eval_last_error — before the device
 * is touched (the addresses are invented and never dereferenced).  Built by tests/test_policy_eval_args_sanitized.py with
 * AddressSanitizer + UBSan against the sanitized library, so the host validation — the range arithmetic at the 2^40 bound and at the
 * top of the address space, the alignment and overlap loops over inputs and outputs, the thread-local error slot — runs instrumented. */
#include <stdio.h>
#include <string.h>

#include "mxv_policy.h"
#include "mxv_policy_eval.h"

#define P(x) ((void *)(uintptr_t)(x))
#define M 0x100000ull
static int calls = 0, bad = 0;

static void expect(int rc, const char *api, const char *what) {
    const char *msg = mxv_policy_eval_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what) || strncmp(msg, api, strlen(api)) != 0 || msg[strlen(api)] != ':') {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s: ... %s'\n", rc, msg ? msg : "(null)", api, what);
    }
}

#define CF "mxv_policy_eval_categorical"
#define CB "mxv_policy_eval_categorical_backward"
#define GF "mxv_policy_eval_gaussian"
#define GB "mxv_policy_eval_gaussian_backward"

/* logits M, actions 2M, log_prob 3M, entropy 4M */
static int cf(int64_t n, int32_t a, void *x, int64_t ld, void *act, int32_t i64, void *lp, void *en) {
    return mxv_policy_eval_categorical(NULL, n, a, (const float *)x, ld, act, i64, (float *)lp, (float *)en);
}
/* logits M, actions 2M, grad_log_prob 3M, grad_entropy 4M, grad_logits 5M */
static int cb(int64_t n, int32_t a, void *x, int64_t ld, void *act, int32_t i64, void *gl, void *gh, void *g, int64_t gld) {
    return mxv_policy_eval_categorical_backward(NULL, n, a, (const float *)x, ld, act, i64, (const float *)gl, (const float *)gh, (float *)g, gld);
}
/* mean M, log_std 2M, actions 3M, log_prob 4M, entropy 5M */
static int gf(int64_t n, int32_t d, void *mu, int64_t mld, void *ls, int64_t sld, void *act, int64_t ald, void *lp, void *en) {
    return mxv_policy_eval_gaussian(NULL, n, d, (const float *)mu, mld, (const float *)ls, sld, (const float *)act, ald, (float *)lp, (float *)en);
}
/* mean M, log_std 2M, actions 3M, grad_log_prob 4M, grad_entropy 5M, grad_mean 6M, grad_log_std 7M */
static int gb(int64_t n, int32_t d, void *mu, int64_t mld, void *ls, int64_t sld, void *act, int64_t ald, void *gl, void *gh, void *gm, int64_t gmld,
              void *gs, int64_t gsld) {
    return mxv_policy_eval_gaussian_backward(NULL, n, d, (const float *)mu, mld, (const float *)ls, sld, (const float *)act, ald, (const float *)gl,
                                             (const float *)gh, (float *)gm, gmld, (float *)gs, gsld);
}

int main(void) {
    const int64_t big = (int64_t)1 << 62;
    const char *before = mxv_policy_eval_last_error();
    ++calls;
    if (!before || before[0] != '\0') {
        ++bad;
        printf("BAD: the slot is not empty before the first call\n");
    }

    /* ---- categorical, forward ---- */
    expect(cf(16, 3, NULL, 3, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "logits pointer is NULL");
    expect(cf(16, 3, P(M), 3, NULL, 1, P(3 * M), P(4 * M)), CF, "actions pointer is NULL");
    expect(cf(0, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "M =");
    expect(cf(INT64_MIN, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "M =");
    expect(cf(16, 0, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "A =");
    expect(cf(16, 65, P(M), 65, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "A =");
    expect(cf(16, INT32_MIN, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "A =");
    expect(cf(16, 3, P(M), 2, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "ld =");
    expect(cf(16, 3, P(M), -7, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "ld =");
    expect(cf(16, 3, P(M), big, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "2^40");
    expect(cf(big, 3, P(M), INT64_MAX, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "2^40");
    expect(cf(((int64_t)1 << 40) / 3 + 1, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "2^40");
    expect(cf(16, 3, P(M + 2), 3, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "logits pointer");
    expect(cf(16, 3, P(M), 3, P(2 * M + 4), 1, P(3 * M), P(4 * M)), CF, "actions pointer");      /* int64 actions: 8 bytes */
    expect(cf(16, 3, P(M), 3, P(2 * M + 2), 0, P(3 * M), P(4 * M)), CF, "actions pointer");
    expect(cf(16, 3, P(M), 3, P(2 * M), 1, P(3 * M + 1), P(4 * M)), CF, "log_prob pointer");
    expect(cf(16, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M + 3)), CF, "entropy pointer");
    expect(cf(16, 3, P(UINTPTR_MAX - 7), 3, P(2 * M), 1, P(3 * M), P(4 * M)), CF, "address space");
    expect(cf(16, 3, P(M), 3, P(UINTPTR_MAX - 15), 1, P(3 * M), P(4 * M)), CF, "address space");
    expect(cf(16, 3, P(M), 3, P(2 * M), 1, P(UINTPTR_MAX - 3), P(4 * M)), CF, "address space");
    expect(cf(16, 3, P(M), 3, P(2 * M), 1, NULL, P(UINTPTR_MAX - 7)), CF, "address space");
    expect(cf(16, 3, P(M), 3, P(2 * M), 1, P(M + 188), P(4 * M)), CF, "log_prob overlaps the logits");
    expect(cf(16, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(M - 60)), CF, "entropy overlaps the logits");
    expect(cf(16, 3, P(M), 3, P(2 * M), 1, P(2 * M + 124), P(4 * M)), CF, "log_prob overlaps the actions");
    expect(cf(16, 3, P(M), 3, P(2 * M), 0, NULL, P(2 * M + 60)), CF, "entropy overlaps the actions");
    expect(cf(16, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(3 * M + 60)), CF, "outputs log_prob and entropy overlap");

    /* ---- categorical, backward ---- */
    expect(cb(16, 3, NULL, 3, P(2 * M), 1, P(3 * M), P(4 * M), P(5 * M), 3), CB, "logits pointer is NULL");
    expect(cb(16, 3, P(M), 3, NULL, 1, P(3 * M), P(4 * M), P(5 * M), 3), CB, "actions pointer is NULL");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M), NULL, 3), CB, "grad_logits pointer is NULL");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, NULL, NULL, P(5 * M), 3), CB, "both NULL");
    expect(cb(-1, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M), P(5 * M), 3), CB, "M =");
    expect(cb(16, 65, P(M), 65, P(2 * M), 1, P(3 * M), P(4 * M), P(5 * M), 65), CB, "A =");
    expect(cb(16, 3, P(M), 2, P(2 * M), 1, P(3 * M), P(4 * M), P(5 * M), 3), CB, "ld =");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M), P(5 * M), 2), CB, "grad_ld =");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M), P(5 * M), 0), CB, "grad_ld =");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M), P(5 * M), big), CB, "2^40");
    expect(cb(16, 3, P(M), big, P(2 * M), 1, P(3 * M), P(4 * M), P(5 * M), 3), CB, "2^40");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, P(3 * M + 2), P(4 * M), P(5 * M), 3), CB, "grad_log_prob pointer");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, NULL, P(4 * M + 1), P(5 * M), 3), CB, "grad_entropy pointer");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, P(3 * M), NULL, P(5 * M + 2), 3), CB, "grad_logits pointer");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, P(UINTPTR_MAX - 3), NULL, P(5 * M), 3), CB, "address space");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M), P(UINTPTR_MAX - 15), 3), CB, "address space");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M), P(M + 188), 3), CB, "grad_logits overlaps the logits");
    expect(cb(16, 3, P(M), 8, P(2 * M), 1, P(3 * M), P(4 * M), P(M + 12), 8), CB, "grad_logits overlaps the logits");   /* column blocks are not told apart */
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M), P(2 * M - 188), 3), CB, "grad_logits overlaps the actions");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, P(3 * M), P(4 * M), P(3 * M + 60), 3), CB, "grad_logits overlaps the grad_log_prob");
    expect(cb(16, 3, P(M), 3, P(2 * M), 1, NULL, P(4 * M), P(4 * M - 188), 3), CB, "grad_logits overlaps the grad_entropy");

    /* ---- Gaussian, forward ---- */
    expect(gf(16, 3, NULL, 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M)), GF, "mean pointer is NULL");
    expect(gf(16, 3, P(M), 3, NULL, 3, P(3 * M), 3, P(4 * M), P(5 * M)), GF, "log_std pointer is NULL");
    expect(gf(16, 3, P(M), 3, P(2 * M), 3, NULL, 3, P(4 * M), P(5 * M)), GF, "actions pointer is NULL");
    expect(gf(0, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M)), GF, "M =");
    expect(gf(16, 0, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M)), GF, "D =");
    expect(gf(16, 5, P(M), 5, P(2 * M), 5, P(3 * M), 5, P(4 * M), P(5 * M)), GF, "D =");
    expect(gf(16, 3, P(M), 2, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M)), GF, "mean_ld =");
    expect(gf(16, 3, P(M), 3, P(2 * M), 2, P(3 * M), 3, P(4 * M), P(5 * M)), GF, "log_std_ld =");
    expect(gf(16, 3, P(M), 3, P(2 * M), -1, P(3 * M), 3, P(4 * M), P(5 * M)), GF, "log_std_ld =");
    expect(gf(16, 3, P(M), 3, P(2 * M), 0, P(3 * M), 0, P(4 * M), P(5 * M)), GF, "actions_ld =");
    expect(gf(16, 3, P(M), big, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M)), GF, "2^40");
    expect(gf(16, 3, P(M), 3, P(2 * M), 0, P(3 * M), INT64_MAX, P(4 * M), P(5 * M)), GF, "2^40");
    expect(gf(16, 3, P(M + 2), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M)), GF, "mean pointer");
    expect(gf(16, 3, P(M), 3, P(2 * M + 1), 0, P(3 * M), 3, P(4 * M), P(5 * M)), GF, "log_std pointer");
    expect(gf(16, 3, P(M), 3, P(2 * M), 3, P(3 * M + 2), 3, P(4 * M), P(5 * M)), GF, "actions pointer");
    expect(gf(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M + 1), P(5 * M)), GF, "log_prob pointer");
    expect(gf(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M + 3)), GF, "entropy pointer");
    expect(gf(16, 3, P(M), 3, P(UINTPTR_MAX - 7), 0, P(3 * M), 3, P(4 * M), P(5 * M)), GF, "address space");
    expect(gf(16, 3, P(M), 3, P(2 * M), 3, P(UINTPTR_MAX - 15), 3, P(4 * M), P(5 * M)), GF, "address space");
    expect(gf(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(M + 188), P(5 * M)), GF, "log_prob overlaps the mean");
    expect(gf(16, 3, P(M), 3, P(2 * M), 0, P(3 * M), 3, P(2 * M + 8), P(5 * M)), GF, "log_prob overlaps the log_std");
    expect(gf(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(3 * M - 60)), GF, "entropy overlaps the actions");
    expect(gf(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(4 * M + 60)), GF, "outputs log_prob and entropy overlap");

    /* ---- Gaussian, backward ---- */
    expect(gb(16, 3, NULL, 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M), P(6 * M), 3, P(7 * M), 3), GB, "mean pointer is NULL");
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, NULL, NULL, P(6 * M), 3, P(7 * M), 3), GB, "both NULL");
    expect(gb(16, 5, P(M), 5, P(2 * M), 5, P(3 * M), 5, P(4 * M), P(5 * M), P(6 * M), 5, P(7 * M), 5), GB, "D =");
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M), P(6 * M), 2, P(7 * M), 3), GB, "grad_mean_ld =");
    expect(gb(16, 3, P(M), 3, P(2 * M), 0, P(3 * M), 3, P(4 * M), P(5 * M), P(6 * M), 3, P(7 * M), 0), GB, "grad_log_std_ld =");   /* always per row */
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M), P(6 * M), big, P(7 * M), 3), GB, "2^40");
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M), NULL, 0, P(7 * M), INT64_MAX), GB, "2^40");
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M + 2), P(5 * M), P(6 * M), 3, P(7 * M), 3), GB, "grad_log_prob pointer");
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M), P(6 * M + 1), 3, P(7 * M), 3), GB, "grad_mean pointer");
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M), P(6 * M), 3, P(7 * M + 2), 3), GB, "grad_log_std pointer");
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M), P(UINTPTR_MAX - 15), 3, NULL, 0), GB, "address space");
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M), P(M + 188), 3, P(7 * M), 3), GB, "grad_mean overlaps the mean");
    expect(gb(16, 3, P(M), 3, P(2 * M), 0, P(3 * M), 3, P(4 * M), P(5 * M), P(6 * M), 3, P(2 * M + 8), 3), GB, "grad_log_std overlaps the log_std");
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M), P(3 * M - 188), 3, P(7 * M), 3), GB, "grad_mean overlaps the actions");
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M), P(6 * M), 3, P(4 * M + 60), 3), GB, "grad_log_std overlaps the grad_log_prob");
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, NULL, P(5 * M), P(5 * M - 188), 3, NULL, 0), GB, "grad_mean overlaps the grad_entropy");
    expect(gb(16, 3, P(M), 3, P(2 * M), 3, P(3 * M), 3, P(4 * M), P(5 * M), P(6 * M), 3, P(6 * M + 188), 3), GB, "outputs grad_mean and grad_log_std overlap");

    /* the slot is this header's own: a refusal of a sampling call lands in mxv_policy_last_error and leaves this one alone */
    ++calls;
    if (mxv_policy_sample_categorical(NULL, 0, 3, (const float *)P(M), 3, 1u, 2u, 3u, NULL, P(3 * M), 1, NULL, NULL) != MXV_ERR_INVALID_ARG ||
        !strstr(mxv_policy_last_error(), "mxv_policy_sample_categorical") || !strstr(mxv_policy_eval_last_error(), GB)) {
        ++bad;
        printf("BAD: the two headers' error slots are not separate: '%s' / '%s'\n", mxv_policy_last_error(), mxv_policy_eval_last_error());
    }
    printf("policy_eval_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
