/* The argument checks of include/mxv_gae.h driven from plain C: every call below must be refused with MXV_ERR_INVALID_ARG and a
 * message before the device is touched (the addresses are invented and never dereferenced).  Built by tests/test_gae_args_sanitized.py
 * with AddressSanitizer + UBSan against the sanitized library, so the host validation — span arithmetic at the 2^40 bound and at the
 * top of the address space, the alignment loop, the thread-local error slot — runs instrumented. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "mxv_gae.h"

#define P(x) ((void *)(uintptr_t)(x))
#define A 0x100000ull
static int calls = 0, bad = 0;

static void expect(int rc, const char *what) {
    const char *msg = mxv_gae_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what)) {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s'\n", rc, msg ? msg : "(null)", what);
    }
}

static int gae(int64_t K, int64_t N, void *rew, int f64, int64_t ld, void *te, void *tr, void *v, void *lv, void *fv, double g, double l,
               void *adv, void *ret, int64_t ldo) {
    return mxv_gae(NULL, K, N, rew, f64, ld, (const uint8_t *)te, (const uint8_t *)tr, (const float *)v, (const float *)lv, (const float *)fv,
                   g, l, (float *)adv, (float *)ret, ldo);
}

static int rtg(int64_t K, int64_t N, void *rew, int f64, int64_t ld, void *te, void *tr, void *lv, void *fv, double g, void *ret, int64_t ldo) {
    return mxv_discounted_returns(NULL, K, N, rew, f64, ld, (const uint8_t *)te, (const uint8_t *)tr, (const float *)lv, (const float *)fv, g,
                                  (float *)ret, ldo);
}

int main(void) {
    const int64_t big = (int64_t)1 << 62;
    int32_t v;
    uint32_t grid;
    expect(gae(8, 16, NULL, 0, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 16), "reward");
    expect(gae(8, 16, P(A), 0, 16, NULL, P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 16), "terminated");
    expect(gae(8, 16, P(A), 0, 16, P(2 * A), NULL, P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 16), "truncated");
    expect(gae(8, 16, P(A), 0, 16, P(2 * A), P(3 * A), NULL, NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 16), "values");
    expect(gae(8, 16, P(A), 0, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, NULL, P(8 * A), 16), "advantages");
    expect(gae(8, 16, P(A), 0, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), NULL, 16), "returns");
    expect(gae(0, 16, P(A), 0, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 16), "K");
    expect(gae(INT64_MIN, 16, P(A), 0, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 16), "K");
    expect(gae(8, -1, P(A), 0, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 16), "N");
    expect(gae(8, 16, P(A), 0, 15, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 16), "ld");
    expect(gae(8, 16, P(A), 0, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 15), "ld_out");
    expect(gae(8, 16, P(A), 0, big, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 16), "2^40");
    expect(gae(big, big, P(A), 1, INT64_MAX, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), INT64_MAX), "2^40");
    expect(gae((int64_t)1 << 40, 1, P(A), 0, 2, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 1), "2^40");
    expect(gae(8, 16, P(A), 0, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, NAN, 0.9, P(7 * A), P(8 * A), 16), "gamma");
    expect(gae(8, 16, P(A), 0, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, INFINITY, P(7 * A), P(8 * A), 16), "lam");
    expect(gae(8, 16, P(A + 4), 1, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 16), "aligned");
    expect(gae(8, 16, P(A), 0, 16, P(2 * A), P(3 * A), P(4 * A), P(5 * A + 1), NULL, 0.9, 0.9, P(7 * A), P(8 * A), 16), "aligned");
    expect(gae(8, 16, P(A), 0, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(7 * A + 4), 16), "outputs advantages and returns overlap");
    expect(gae(8, 16, P(A), 0, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(4 * A + 64), P(8 * A), 16), "overlaps input values");
    expect(gae(8, 16, P(A), 0, 64, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(A + 4 * 56), P(8 * A), 64), "overlaps input reward");
    /* ranges that would wrap past the top of the address space */
    expect(gae(8, 16, P(UINTPTR_MAX - 7), 1, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(8 * A), 16), "address space");
    expect(gae(8, 16, P(A), 0, 16, P(2 * A), P(3 * A), P(4 * A), NULL, NULL, 0.9, 0.9, P(7 * A), P(UINTPTR_MAX - 3), 16), "address space");
    expect(rtg(8, 16, NULL, 1, 16, P(2 * A), P(3 * A), NULL, NULL, 0.9, P(8 * A), 16), "reward");
    expect(rtg(8, 16, P(A), 1, 16, P(2 * A), P(3 * A), NULL, NULL, 0.9, NULL, 16), "returns");
    expect(rtg(8, 16, P(A), 1, 16, P(2 * A), P(3 * A), NULL, NULL, -INFINITY, P(8 * A), 16), "gamma");
    expect(rtg(8, 16, P(A), 1, 16, P(2 * A), P(3 * A), NULL, NULL, 0.9, P(3 * A - 4), 16), "overlaps input truncated");
    expect(rtg(8, 16, P(A), 1, 16, P(2 * A), P(3 * A), P(8 * A + 160), NULL, 0.9, P(8 * A), 16), "overlaps input last_value");
    expect(rtg(8, 16, P(A), 1, 16, P(2 * A), P(3 * A), NULL, P(8 * A - 400), 0.9, P(8 * A), 16), "overlaps input final_values");
    expect(mxv_gae_last_launch(NULL, &grid), "mxv_gae_last_launch");
    expect(mxv_gae_last_launch(&v, NULL), "mxv_gae_last_launch");
    ++calls;
    if (mxv_gae_last_launch(&v, &grid) != MXV_OK || v != 0 || grid != 0) {
        ++bad;
        printf("BAD: a launch was recorded (%d, %u)\n", v, grid);
    }
    printf("gae_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
