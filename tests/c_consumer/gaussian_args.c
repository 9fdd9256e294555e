/* The argument checks of mxv_policy_sample_gaussian (include/mxv_policy.h) driven from plain C: every call below must be refused with
 * MXV_ERR_INVALID_ARG and a message — in the error slot the header's calls share, mxv_policy_last_error — before the device is touched
 * (the addresses are invented and never dereferenced).  Built by tests/test_gaussian_args_sanitized.py with AddressSanitizer + UBSan
 * against the sanitized library, so the host validation — the range arithmetic at the 2^40 bound and at the top of the address space,
 * the alignment loop, the thread-local error slot shared by two translation units — runs instrumented. */
#include <stdio.h>
#include <string.h>

#include "mxv_policy.h"

#define P(x) ((void *)(uintptr_t)(x))
#define M 0x100000ull
static int calls = 0, bad = 0;

static void expect(int rc, const char *what) {
    const char *msg = mxv_policy_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what) || !strstr(msg, "mxv_policy_sample_gaussian")) {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s'\n", rc, msg ? msg : "(null)", what);
    }
}

/* mean at `mean` with stride mld, log_std at `ls` with stride sld, actions at `act` with stride ald */
static int draw(int64_t N, int32_t D, void *mean, int64_t mld, void *ls, int64_t sld, void *step_dev, void *act, int64_t ald, void *lp, void *en) {
    return mxv_policy_sample_gaussian(NULL, N, D, (const float *)mean, mld, (const float *)ls, sld, 1u, 2u, 3u, (uint64_t *)step_dev, (float *)act,
                                      ald, (float *)lp, (float *)en);
}

int main(void) {
    const int64_t big = (int64_t)1 << 62;
    /* mean M, log_std 2M, actions 3M, log_prob 4M, entropy 5M, counter 6M */
    expect(draw(16, 3, NULL, 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "mean pointer is NULL");
    expect(draw(16, 3, P(M), 3, NULL, 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "log_std pointer is NULL");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, NULL, 3, P(4 * M), P(5 * M)), "actions pointer is NULL");
    expect(draw(0, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "N =");
    expect(draw(INT64_MIN, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "N =");
    expect(draw(16, 0, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "D =");
    expect(draw(16, 5, P(M), 5, P(2 * M), 5, NULL, P(3 * M), 5, P(4 * M), P(5 * M)), "D =");
    expect(draw(16, INT32_MIN, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "D =");
    expect(draw(16, 3, P(M), 2, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "mean_ld =");
    expect(draw(16, 3, P(M), 0, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "mean_ld =");
    expect(draw(16, 3, P(M), -5, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "mean_ld =");
    expect(draw(16, 3, P(M), 3, P(2 * M), 2, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "log_std_ld =");
    expect(draw(16, 3, P(M), 3, P(2 * M), -1, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "log_std_ld =");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 2, P(4 * M), P(5 * M)), "actions_ld =");
    expect(draw(16, 3, P(M), 3, P(2 * M), 0, NULL, P(3 * M), 0, P(4 * M), P(5 * M)), "actions_ld =");
    expect(draw(16, 3, P(M), big, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "2^40");
    expect(draw(16, 3, P(M), 3, P(2 * M), big, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "2^40");
    expect(draw(16, 3, P(M), 3, P(2 * M), 0, NULL, P(3 * M), INT64_MAX, P(4 * M), P(5 * M)), "2^40");
    expect(draw(big, 3, P(M), INT64_MAX, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "2^40");
    expect(draw(((int64_t)1 << 40) / 3 + 1, 3, P(M), 3, P(2 * M), 0, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "2^40");
    /* pointers off their element's boundary */
    expect(draw(16, 3, P(M + 2), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "mean pointer");
    expect(draw(16, 3, P(M), 3, P(2 * M + 1), 0, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "log_std pointer");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, P(6 * M + 4), P(3 * M), 3, P(4 * M), P(5 * M)), "step_dev pointer");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M + 2), 3, P(4 * M), P(5 * M)), "actions pointer");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M + 1), P(5 * M)), "log_prob pointer");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M + 3)), "entropy pointer");
    /* ranges that would wrap past the top of the address space */
    expect(draw(16, 3, P(UINTPTR_MAX - 7), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "address space");
    expect(draw(16, 3, P(M), 3, P(UINTPTR_MAX - 7), 0, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "address space");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(UINTPTR_MAX - 15), 3, P(4 * M), P(5 * M)), "address space");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(UINTPTR_MAX - 3), P(5 * M)), "address space");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, NULL, P(UINTPTR_MAX - 7)), "address space");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, P(UINTPTR_MAX - 7), P(3 * M), 3, NULL, NULL), "address space");
    /* an output that shares a byte with the mean, with the log_std, with step_dev or with another output */
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(M + 188), 3, P(4 * M), P(5 * M)), "actions overlaps the mean");
    expect(draw(16, 3, P(M), 8, P(2 * M), 3, NULL, P(3 * M), 3, P(M + 4 * 122), NULL), "log_prob overlaps the mean");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, NULL, P(M - 60)), "entropy overlaps the mean");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(2 * M - 188), 3, P(4 * M), P(5 * M)), "actions overlaps the log_std");
    expect(draw(16, 3, P(M), 3, P(2 * M), 0, NULL, P(3 * M), 3, P(2 * M + 8), P(5 * M)), "log_prob overlaps the log_std");
    expect(draw(16, 3, P(M), 3, P(2 * M), 5, NULL, P(3 * M), 3, P(4 * M), P(2 * M + 4 * 77)), "entropy overlaps the log_std");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, P(3 * M + 184), P(3 * M), 3, P(4 * M), P(5 * M)), "actions overlaps step_dev");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, P(4 * M), P(3 * M), 3, P(4 * M + 4), P(5 * M)), "log_prob overlaps step_dev");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, P(5 * M + 56), P(3 * M), 3, P(4 * M), P(5 * M)), "entropy overlaps step_dev");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(3 * M + 188), P(5 * M)), "outputs actions and log_prob overlap");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 7, P(4 * M), P(3 * M + 4 * 107)), "outputs actions and entropy overlap");
    expect(draw(16, 3, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(4 * M + 60)), "outputs log_prob and entropy overlap");
    /* the slot is the one of the categorical call: its refusal replaces the message above, and the other way round */
    ++calls;
    if (mxv_policy_sample_categorical(NULL, 0, 3, (const float *)P(M), 3, 1u, 2u, 3u, NULL, P(3 * M), 1, NULL, NULL) != MXV_ERR_INVALID_ARG ||
        !strstr(mxv_policy_last_error(), "mxv_policy_sample_categorical")) {
        ++bad;
        printf("BAD: the categorical call's message did not reach the shared slot: '%s'\n", mxv_policy_last_error());
    }
    expect(draw(16, 0, P(M), 3, P(2 * M), 3, NULL, P(3 * M), 3, P(4 * M), P(5 * M)), "D =");
    printf("gaussian_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
