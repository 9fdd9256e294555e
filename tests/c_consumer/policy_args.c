/* The argument checks of include/mxv_policy.h driven from plain C: every call below must be refused with MXV_ERR_INVALID_ARG and a
 * message before the device is touched (the addresses are invented and never dereferenced).  Built by
 * tests/test_policy_args_sanitized.py with AddressSanitizer + UBSan against the sanitized library, so the host validation — the range
 * arithmetic at the 2^40 bound and at the top of the address space, the alignment loop, the thread-local error slot — runs
 * instrumented. */
#include <stdio.h>
#include <string.h>

#include "mxv_policy.h"

#define P(x) ((void *)(uintptr_t)(x))
#define M 0x100000ull
static int calls = 0, bad = 0;

static void expect(int rc, const char *what) {
    const char *msg = mxv_policy_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what)) {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s'\n", rc, msg ? msg : "(null)", what);
    }
}

static int draw(int64_t N, int32_t A, void *logits, int64_t ld, void *step_dev, void *actions, int i64, void *lp, void *en) {
    return mxv_policy_sample_categorical(NULL, N, A, (const float *)logits, ld, 1u, 2u, 3u, (uint64_t *)step_dev, actions, i64, (float *)lp,
                                         (float *)en);
}

int main(void) {
    const int64_t big = (int64_t)1 << 62;
    int32_t v, a;
    uint32_t grid;
    expect(draw(16, 3, NULL, 3, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "logits pointer is NULL");
    expect(draw(16, 3, P(M), 3, NULL, NULL, 1, P(3 * M), P(4 * M)), "actions pointer is NULL");
    expect(draw(0, 3, P(M), 3, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "N =");
    expect(draw(INT64_MIN, 3, P(M), 3, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "N =");
    expect(draw(16, 0, P(M), 3, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "A =");
    expect(draw(16, 65, P(M), 65, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "A =");
    expect(draw(16, INT32_MIN, P(M), 3, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "A =");
    expect(draw(16, 3, P(M), 2, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "ld =");
    expect(draw(16, 3, P(M), -5, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "ld =");
    expect(draw(16, 3, P(M), big, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "2^40");
    expect(draw(big, 3, P(M), INT64_MAX, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "2^40");
    expect(draw(((int64_t)1 << 40) / 3 + 1, 3, P(M), 3, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "2^40");
    /* pointers off their element's boundary */
    expect(draw(16, 3, P(M + 2), 3, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "logits pointer");
    expect(draw(16, 3, P(M), 3, P(5 * M + 4), P(2 * M), 1, P(3 * M), P(4 * M)), "step_dev pointer");
    expect(draw(16, 3, P(M), 3, NULL, P(2 * M + 4), 1, P(3 * M), P(4 * M)), "actions pointer");
    expect(draw(16, 3, P(M), 3, NULL, P(2 * M + 2), 0, P(3 * M), P(4 * M)), "actions pointer");
    expect(draw(16, 3, P(M), 3, NULL, P(2 * M), 1, P(3 * M + 1), P(4 * M)), "log_prob pointer");
    expect(draw(16, 3, P(M), 3, NULL, P(2 * M), 1, P(3 * M), P(4 * M + 3)), "entropy pointer");
    /* ranges that would wrap past the top of the address space */
    expect(draw(16, 3, P(UINTPTR_MAX - 7), 3, NULL, P(2 * M), 1, P(3 * M), P(4 * M)), "address space");
    expect(draw(16, 3, P(M), 3, NULL, P(UINTPTR_MAX - 15), 1, P(3 * M), P(4 * M)), "address space");
    expect(draw(16, 3, P(M), 3, NULL, P(2 * M), 1, P(UINTPTR_MAX - 3), P(4 * M)), "address space");
    expect(draw(16, 3, P(M), 3, NULL, P(2 * M), 1, NULL, P(UINTPTR_MAX - 7)), "address space");
    expect(draw(16, 3, P(M), 3, P(UINTPTR_MAX - 7), P(2 * M), 1, NULL, NULL), "address space");
    /* an output that shares a byte with the logits, with step_dev or with another output */
    expect(draw(16, 3, P(M), 3, NULL, P(M + 184), 1, P(3 * M), P(4 * M)), "actions overlaps the logits");
    expect(draw(16, 3, P(M), 8, NULL, P(2 * M), 1, P(M + 4 * 120), NULL), "log_prob overlaps the logits");
    expect(draw(16, 3, P(M), 3, NULL, P(2 * M), 0, NULL, P(M - 60)), "entropy overlaps the logits");
    expect(draw(16, 3, P(M), 3, P(2 * M + 120), P(2 * M), 1, P(3 * M), P(4 * M)), "actions overlaps step_dev");
    expect(draw(16, 3, P(M), 3, P(3 * M), P(2 * M), 1, P(3 * M + 4), P(4 * M)), "log_prob overlaps step_dev");
    expect(draw(16, 3, P(M), 3, P(4 * M + 56), P(2 * M), 1, P(3 * M), P(4 * M)), "entropy overlaps step_dev");
    expect(draw(16, 3, P(M), 3, NULL, P(2 * M), 1, P(2 * M + 124), P(4 * M)), "outputs actions and log_prob overlap");
    expect(draw(16, 3, P(M), 3, NULL, P(2 * M), 0, P(3 * M), P(2 * M + 60)), "outputs actions and entropy overlap");
    expect(draw(16, 3, P(M), 3, NULL, P(2 * M), 1, P(3 * M), P(3 * M + 60)), "outputs log_prob and entropy overlap");
    expect(mxv_policy_last_launch(NULL, &a, &grid), "mxv_policy_last_launch");
    expect(mxv_policy_last_launch(&v, NULL, &grid), "mxv_policy_last_launch");
    expect(mxv_policy_last_launch(&v, &a, NULL), "mxv_policy_last_launch");
    ++calls;
    if (mxv_policy_last_launch(&v, &a, &grid) != MXV_OK || v != 0 || a != 0 || grid != 0) {
        ++bad;
        printf("BAD: a launch was recorded (%d, %d, %u)\n", v, a, grid);
    }
    printf("policy_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
