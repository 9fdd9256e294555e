/* The argument checks of include/mxv_vtrace.h driven from plain C: every call below must be refused with MXV_ERR_INVALID_ARG and a
 * message naming the argument before the device is touched (the addresses are invented and never dereferenced).  Built by
 * tests/test_vtrace_args.py against the shipped library and, with AddressSanitizer + UBSan, against the sanitized one, so the host
 * validation — span arithmetic at the 2^40 bound and at the top of the address space, the alignment loop, the thread-local error slot —
 * runs instrumented. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "mxv_vtrace.h"

#define P(x) ((void *)(uintptr_t)(x))
#define A 0x100000ull
static int calls = 0, bad = 0;

static void expect(int rc, const char *what) {
    const char *msg = mxv_vtrace_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what) || strncmp(msg, "mxv_vtrace", 10) != 0) {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s'\n", rc, msg ? msg : "(null)", what);
    }
}

/* the arguments of one call; ok() fills in a call that would be accepted */
typedef struct {
    int64_t K, N, ld, ldo;
    void *lp, *old, *rew, *te, *tr, *v, *lv, *fv, *vs, *pg;
    int f64;
    double g, l, rho, c, pgr;
} args;

static args ok(void) {
    args a = {8, 16, 16, 16, P(9 * A), P(10 * A), P(A), P(2 * A), P(3 * A), P(4 * A), NULL, NULL, P(7 * A), P(8 * A), 0, 0.9, 0.9, 1.0, 1.0, 1.0};
    return a;
}

static int vt(args a) {
    return mxv_vtrace(NULL, a.K, a.N, (const float *)a.lp, (const float *)a.old, a.rew, a.f64, a.ld, (const uint8_t *)a.te, (const uint8_t *)a.tr,
                      (const float *)a.v, (const float *)a.lv, (const float *)a.fv, a.g, a.l, a.rho, a.c, a.pgr, (float *)a.vs, (float *)a.pg, a.ldo);
}

#define BAD(change, what) \
    do {                  \
        args a = ok();    \
        change;           \
        expect(vt(a), what); \
    } while (0)

int main(void) {
    const int64_t big = (int64_t)1 << 62;
    int32_t v;
    uint32_t grid;
    BAD(a.lp = NULL, "log_prob pointer is NULL");
    BAD(a.old = NULL, "old_log_prob pointer is NULL");
    BAD(a.rew = NULL, "reward pointer is NULL");
    BAD(a.te = NULL, "terminated pointer is NULL");
    BAD(a.tr = NULL, "truncated pointer is NULL");
    BAD(a.v = NULL, "values pointer is NULL");
    BAD(a.vs = NULL, "vs pointer is NULL");
    BAD(a.pg = NULL, "pg_advantages pointer is NULL");
    BAD(a.K = 0, "K = 0");
    BAD(a.K = INT64_MIN, "K = ");
    BAD(a.N = -1, "N = -1");
    BAD(a.ld = 15, "ld = 15");
    BAD(a.ldo = 15, "ld_out = 15");
    BAD(a.ld = big, "2^40");
    BAD((a.K = big, a.N = big, a.ld = INT64_MAX, a.ldo = INT64_MAX, a.f64 = 1), "2^40");
    BAD((a.K = (int64_t)1 << 40, a.N = 1, a.ld = 2, a.ldo = 1), "2^40");
    BAD(a.g = NAN, "gamma");
    BAD(a.l = INFINITY, "lam");
    BAD(a.rho = NAN, "rho_bar");
    BAD(a.rho = 0.0, "rho_bar");
    BAD(a.rho = INFINITY, "rho_bar");
    BAD(a.c = -1.0, "c_bar");
    BAD(a.c = -INFINITY, "c_bar");
    BAD(a.pgr = 0.0, "pg_rho_bar");
    BAD(a.pgr = NAN, "pg_rho_bar");
    BAD(a.lp = P(9 * A + 2), "log_prob pointer");
    BAD(a.old = P(10 * A + 1), "old_log_prob pointer");
    BAD((a.rew = P(A + 4), a.f64 = 1), "reward pointer");
    BAD(a.v = P(4 * A + 3), "values pointer");
    BAD(a.lv = P(5 * A + 1), "last_value pointer");
    BAD(a.fv = P(6 * A + 2), "final_values pointer");
    BAD(a.vs = P(7 * A + 1), "vs pointer");
    BAD(a.pg = P(8 * A + 2), "pg_advantages pointer");
    BAD(a.pg = P(7 * A + 4), "outputs vs and pg_advantages overlap");
    BAD(a.vs = P(9 * A + 64), "output vs overlaps input log_prob");
    BAD(a.pg = P(10 * A), "output pg_advantages overlaps input old_log_prob");
    BAD(a.vs = P(4 * A + 64), "overlaps input values");
    BAD(a.pg = P(2 * A + 8 * 16 - 4), "overlaps input terminated");
    BAD(a.vs = P(3 * A - 4), "overlaps input truncated");
    BAD(a.lv = P(8 * A + 160), "overlaps input last_value");
    BAD(a.fv = P(8 * A - 400), "overlaps input final_values");
    BAD((a.ld = 64, a.ldo = 64, a.vs = P(A + 4 * 56)), "overlaps input reward");        /* the block wraps into the next row's reward */
    BAD((a.ld = 64, a.ldo = 48, a.vs = P(A + 4 * 16)), "overlaps input reward");        /* interleaved with another row stride */
    /* ranges that would wrap past the top of the address space */
    BAD((a.rew = P(UINTPTR_MAX - 7), a.f64 = 1), "address space");
    BAD(a.lp = P(UINTPTR_MAX - 3), "address space");
    BAD(a.pg = P(UINTPTR_MAX - 3), "address space");
    expect(mxv_vtrace_last_launch(NULL, &grid), "mxv_vtrace_last_launch");
    expect(mxv_vtrace_last_launch(&v, NULL), "mxv_vtrace_last_launch");
    ++calls;
    if (mxv_vtrace_last_launch(&v, &grid) != MXV_OK || v != 0 || grid != 0) {
        ++bad;
        printf("BAD: a launch was recorded (%d, %u)\n", v, grid);
    }
    printf("vtrace_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
