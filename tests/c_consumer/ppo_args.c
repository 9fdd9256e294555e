/* The argument checks of the calls of include/mxv_ppo.h driven from plain C: every call below must be refused with MXV_ERR_INVALID_ARG and
 * a message that names the call — in the header's own error slot, mxv_ppo_last_error — before the device is touched (the addresses are
 * invented and never dereferenced).  Built by tests/test_ppo_args_sanitized.py with AddressSanitizer + UBSan against the sanitized
 * library, so the host validation — the workspace arithmetic at the 2^40 bound, the range arithmetic at the top of the address space,
 * the alignment and overlap loops over seven inputs and three outputs, the thread-local error slot — runs instrumented. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "mxv_policy_eval.h"
#include "mxv_ppo.h"

#define P(x) ((void *)(uintptr_t)(x))
#define M 0x100000ull
static int calls = 0, bad = 0;

static void expect(int rc, const char *api, const char *what) {
    const char *msg = mxv_ppo_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what) || strncmp(msg, api, strlen(api)) != 0 || msg[strlen(api)] != ':') {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s: ... %s'\n", rc, msg ? msg : "(null)", api, what);
    }
}

#define AM "mxv_ppo_advantage_moments"
#define CL "mxv_ppo_clip_loss"
#define CB "mxv_ppo_clip_loss_backward"
#define WS 64 /* mxv_ppo_workspace_bytes of up to 1024 rows */

/* advantages M, workspace 2M, moments_out 3M */
static int am(int64_t n, void *adv, double eps, void *ws, int64_t wsb, void *out) {
    return mxv_ppo_advantage_moments(NULL, n, (const float *)adv, eps, ws, wsb, (double *)out);
}
/* log_prob M, old 2M, adv 3M, moments 4M, entropy 5M, values 6M, returns 7M, workspace 8M, loss 9M, stats 10M */
static int cl(int64_t n, void *lp, void *old, void *adv, void *mom, void *en, void *v, void *ret, double clip, double ec, double vc, void *ws,
              int64_t wsb, void *loss, void *stats) {
    return mxv_ppo_clip_loss(NULL, n, (const float *)lp, (const float *)old, (const float *)adv, (const double *)mom, (const float *)en,
                             (const float *)v, (const float *)ret, clip, ec, vc, ws, wsb, (float *)loss, (float *)stats);
}
/* the same inputs; grad_loss 8M, grad_log_prob 9M, grad_entropy 10M, grad_values 11M */
static int cb(int64_t n, void *lp, void *old, void *adv, void *mom, void *en, void *v, void *ret, double clip, double ec, double vc, void *g,
              void *glp, void *gen, void *gv) {
    return mxv_ppo_clip_loss_backward(NULL, n, (const float *)lp, (const float *)old, (const float *)adv, (const double *)mom,
                                      (const float *)en, (const float *)v, (const float *)ret, clip, ec, vc, (const float *)g, (float *)glp,
                                      (float *)gen, (float *)gv);
}

int main(void) {
    const int64_t big = (int64_t)1 << 40;
    const char *before = mxv_ppo_last_error();
    ++calls;
    if (!before || before[0] != '\0') {
        ++bad;
        printf("BAD: the slot is not empty before the first call\n");
    }

    /* ---- the workspace size: no status, 0 outside 1..2^40 ---- */
    ++calls;
    if (mxv_ppo_workspace_bytes(0) != 0 || mxv_ppo_workspace_bytes(-5) != 0 || mxv_ppo_workspace_bytes(INT64_MIN) != 0 ||
        mxv_ppo_workspace_bytes(big + 1) != 0 || mxv_ppo_workspace_bytes(INT64_MAX) != 0 || mxv_ppo_workspace_bytes(1) != WS ||
        mxv_ppo_workspace_bytes(1024) != WS || mxv_ppo_workspace_bytes(1025) != 2 * WS || mxv_ppo_workspace_bytes(1 << 20) != 1024 * WS ||
        mxv_ppo_workspace_bytes((1 << 20) + 1) != (1025 + 2) * WS || mxv_ppo_workspace_bytes(big) != (((int64_t)1 << 30) + (1 << 20) + 1024) * WS) {
        ++bad;
        printf("BAD: mxv_ppo_workspace_bytes\n");
    }

    /* ---- advantage moments ---- */
    expect(am(16, NULL, 1e-8, P(2 * M), WS, P(3 * M)), AM, "advantages pointer is NULL");
    expect(am(16, P(M), 1e-8, NULL, WS, P(3 * M)), AM, "workspace pointer is NULL");
    expect(am(16, P(M), 1e-8, P(2 * M), WS, NULL), AM, "moments_out pointer is NULL");
    expect(am(0, P(M), 1e-8, P(2 * M), WS, P(3 * M)), AM, "M =");
    expect(am(INT64_MIN, P(M), 1e-8, P(2 * M), WS, P(3 * M)), AM, "M =");
    expect(am(big + 1, P(M), 1e-8, P(2 * M), INT64_MAX, P(3 * M)), AM, "2^40");
    expect(am(INT64_MAX, P(M), 1e-8, P(2 * M), INT64_MAX, P(3 * M)), AM, "2^40");
    expect(am(16, P(M), -1e-8, P(2 * M), WS, P(3 * M)), AM, "eps =");
    expect(am(16, P(M), NAN, P(2 * M), WS, P(3 * M)), AM, "eps =");
    expect(am(16, P(M), INFINITY, P(2 * M), WS, P(3 * M)), AM, "eps =");
    expect(am(16, P(M), 1e-8, P(2 * M), WS - 1, P(3 * M)), AM, "workspace_bytes =");
    expect(am(16, P(M), 1e-8, P(2 * M), 0, P(3 * M)), AM, "workspace_bytes =");
    expect(am(16, P(M), 1e-8, P(2 * M), -WS, P(3 * M)), AM, "workspace_bytes =");
    expect(am(1025, P(M), 1e-8, P(2 * M), WS, P(3 * M)), AM, "workspace_bytes =");
    expect(am(16, P(M), 1e-8, P(2 * M + 4), WS, P(3 * M)), AM, "workspace pointer");
    expect(am(16, P(M + 2), 1e-8, P(2 * M), WS, P(3 * M)), AM, "advantages pointer");
    expect(am(16, P(M), 1e-8, P(2 * M), WS, P(3 * M + 4)), AM, "moments_out pointer");
    expect(am(16, P(UINTPTR_MAX - 7), 1e-8, P(2 * M), WS, P(3 * M)), AM, "address space");
    expect(am(16, P(M), 1e-8, P(UINTPTR_MAX - 15), WS, P(3 * M)), AM, "address space");
    expect(am(16, P(M), 1e-8, P(2 * M), WS, P(UINTPTR_MAX - 7)), AM, "address space");
    expect(am(16, P(M), 1e-8, P(M + 56), WS, P(3 * M)), AM, "workspace overlaps the advantages");
    expect(am(16, P(M), 1e-8, P(2 * M), WS, P(M - 8)), AM, "moments_out overlaps the advantages");
    expect(am(16, P(M), 1e-8, P(2 * M), WS, P(2 * M + 56)), AM, "outputs workspace and moments_out overlap");

    /* ---- the loss, forward ---- */
#define CLOK P(M), P(2 * M), P(3 * M), P(4 * M), P(5 * M), P(6 * M), P(7 * M)
    expect(cl(16, NULL, P(2 * M), P(3 * M), P(4 * M), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "log_prob pointer is NULL");
    expect(cl(16, P(M), NULL, P(3 * M), P(4 * M), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "old_log_prob pointer is NULL");
    expect(cl(16, P(M), P(2 * M), NULL, P(4 * M), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "advantages pointer is NULL");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, NULL, WS, P(9 * M), P(10 * M)), CL, "workspace pointer is NULL");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, NULL, P(10 * M)), CL, "loss_out pointer is NULL");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), NULL), CL, "stats_out pointer is NULL");
    expect(cl(0, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "M =");
    expect(cl(-3, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "M =");
    expect(cl(big + 1, CLOK, 0.2, 0.01, 0.5, P(8 * M), INT64_MAX, P(9 * M), P(10 * M)), CL, "2^40");
    expect(cl(16, P(M), P(2 * M), P(3 * M), P(4 * M), P(5 * M), P(6 * M), NULL, 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "values and returns");
    expect(cl(16, P(M), P(2 * M), P(3 * M), P(4 * M), P(5 * M), NULL, P(7 * M), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "values and returns");
    expect(cl(16, CLOK, 1.0, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "clip =");
    expect(cl(16, CLOK, -0.001, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "clip =");
    expect(cl(16, CLOK, NAN, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "clip =");
    expect(cl(16, CLOK, 0.2, INFINITY, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "entropy_coef =");
    expect(cl(16, CLOK, 0.2, 0.01, NAN, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "value_coef =");
    expect(cl(16, CLOK, 0.2, 0.01, -INFINITY, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "value_coef =");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS - 8, P(9 * M), P(10 * M)), CL, "workspace_bytes =");
    expect(cl(1 << 20, P(M), P(6 * M), P(11 * M), NULL, NULL, NULL, NULL, 0.2, 0.01, 0.5, P(16 * M), 1023 * WS, P(17 * M), P(18 * M)), CL, "workspace_bytes =");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M + 4), WS, P(9 * M), P(10 * M)), CL, "workspace pointer");
    expect(cl(16, P(M + 1), P(2 * M), P(3 * M), P(4 * M), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "log_prob pointer");
    expect(cl(16, P(M), P(2 * M + 2), P(3 * M), P(4 * M), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "old_log_prob pointer");
    expect(cl(16, P(M), P(2 * M), P(3 * M + 3), P(4 * M), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "advantages pointer");
    expect(cl(16, P(M), P(2 * M), P(3 * M), P(4 * M + 4), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "moments pointer");
    expect(cl(16, P(M), P(2 * M), P(3 * M), P(4 * M), P(5 * M + 2), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "entropy pointer");
    expect(cl(16, P(M), P(2 * M), P(3 * M), P(4 * M), P(5 * M), P(6 * M + 2), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "values pointer");
    expect(cl(16, P(M), P(2 * M), P(3 * M), P(4 * M), P(5 * M), P(6 * M), P(7 * M + 1), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "returns pointer");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M + 2), P(10 * M)), CL, "loss_out pointer");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M + 1)), CL, "stats_out pointer");
    expect(cl(16, P(UINTPTR_MAX - 7), P(2 * M), P(3 * M), P(4 * M), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "address space");
    expect(cl(16, P(M), P(2 * M), P(3 * M), P(UINTPTR_MAX - 7), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(10 * M)), CL, "address space");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(UINTPTR_MAX - 15), WS, P(9 * M), P(10 * M)), CL, "address space");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(UINTPTR_MAX - 15)), CL, "address space");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(M + 56), WS, P(9 * M), P(10 * M)), CL, "workspace overlaps the log_prob");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(2 * M - 56), WS, P(9 * M), P(10 * M)), CL, "workspace overlaps the old_log_prob");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(4 * M + 8), WS, P(9 * M), P(10 * M)), CL, "workspace overlaps the moments");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(3 * M + 60), P(10 * M)), CL, "loss_out overlaps the advantages");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(4 * M + 12), P(10 * M)), CL, "loss_out overlaps the moments");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(5 * M - 28)), CL, "stats_out overlaps the entropy");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(6 * M + 60)), CL, "stats_out overlaps the values");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(7 * M), P(10 * M)), CL, "loss_out overlaps the returns");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(8 * M + 60), P(10 * M)), CL, "outputs workspace and loss_out overlap");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(9 * M), P(8 * M - 4)), CL, "outputs workspace and stats_out overlap");
    expect(cl(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), WS, P(10 * M + 28), P(10 * M)), CL, "outputs loss_out and stats_out overlap");

    /* ---- the loss, backward ---- */
    expect(cb(16, NULL, P(2 * M), P(3 * M), P(4 * M), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), P(9 * M), P(10 * M), P(11 * M)), CB, "log_prob pointer is NULL");
    expect(cb(16, P(M), NULL, P(3 * M), P(4 * M), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), P(9 * M), P(10 * M), P(11 * M)), CB, "old_log_prob pointer is NULL");
    expect(cb(16, P(M), P(2 * M), NULL, P(4 * M), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), P(9 * M), P(10 * M), P(11 * M)), CB, "advantages pointer is NULL");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, NULL, P(9 * M), P(10 * M), P(11 * M)), CB, "grad_loss pointer is NULL");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), NULL, NULL, NULL), CB, "all NULL");
    expect(cb(16, P(M), P(2 * M), P(3 * M), P(4 * M), NULL, P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), P(9 * M), P(10 * M), P(11 * M)), CB, "entropy is NULL");
    expect(cb(16, P(M), P(2 * M), P(3 * M), P(4 * M), P(5 * M), NULL, NULL, 0.2, 0.01, 0.5, P(8 * M), P(9 * M), P(10 * M), P(11 * M)), CB, "values is NULL");
    expect(cb(0, CLOK, 0.2, 0.01, 0.5, P(8 * M), P(9 * M), P(10 * M), P(11 * M)), CB, "M =");
    expect(cb(big + 1, CLOK, 0.2, 0.01, 0.5, P(8 * M), P(9 * M), P(10 * M), P(11 * M)), CB, "2^40");
    expect(cb(16, P(M), P(2 * M), P(3 * M), P(4 * M), P(5 * M), NULL, P(7 * M), 0.2, 0.01, 0.5, P(8 * M), P(9 * M), P(10 * M), NULL), CB, "values and returns");
    expect(cb(16, CLOK, 1.5, 0.01, 0.5, P(8 * M), P(9 * M), P(10 * M), P(11 * M)), CB, "clip =");
    expect(cb(16, CLOK, INFINITY, 0.01, 0.5, P(8 * M), P(9 * M), P(10 * M), P(11 * M)), CB, "clip =");
    expect(cb(16, CLOK, 0.2, NAN, 0.5, P(8 * M), P(9 * M), P(10 * M), P(11 * M)), CB, "entropy_coef =");
    expect(cb(16, CLOK, 0.2, 0.01, INFINITY, P(8 * M), P(9 * M), P(10 * M), P(11 * M)), CB, "value_coef =");
    expect(cb(16, P(M), P(2 * M), P(3 * M), P(4 * M + 2), P(5 * M), P(6 * M), P(7 * M), 0.2, 0.01, 0.5, P(8 * M), P(9 * M), P(10 * M), P(11 * M)), CB, "moments pointer");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M + 2), P(9 * M), P(10 * M), P(11 * M)), CB, "grad_loss pointer");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), P(9 * M + 1), P(10 * M), P(11 * M)), CB, "grad_log_prob pointer");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), NULL, P(10 * M + 2), P(11 * M)), CB, "grad_entropy pointer");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), NULL, NULL, P(11 * M + 3)), CB, "grad_values pointer");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(UINTPTR_MAX - 3), P(9 * M), P(10 * M), P(11 * M)), CB, "address space");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), P(UINTPTR_MAX - 15), NULL, NULL), CB, "address space");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), P(M + 60), P(10 * M), P(11 * M)), CB, "grad_log_prob overlaps the log_prob");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), P(9 * M), P(5 * M - 60), P(11 * M)), CB, "grad_entropy overlaps the entropy");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), P(9 * M), P(10 * M), P(7 * M - 4)), CB, "grad_values overlaps the returns");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), P(8 * M - 60), NULL, NULL), CB, "grad_log_prob overlaps the grad_loss");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), P(4 * M + 12), NULL, NULL), CB, "grad_log_prob overlaps the moments");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), P(9 * M), P(9 * M + 60), P(11 * M)), CB, "outputs grad_log_prob and grad_entropy overlap");
    expect(cb(16, CLOK, 0.2, 0.01, 0.5, P(8 * M), NULL, P(10 * M), P(10 * M - 60)), CB, "outputs grad_entropy and grad_values overlap");

    /* the slot is this header's own: a refusal of an evaluation call lands in mxv_policy_eval_last_error and leaves this one alone */
    ++calls;
    if (mxv_policy_eval_categorical(NULL, 0, 3, (const float *)P(M), 3, P(2 * M), 1, (float *)P(3 * M), (float *)P(4 * M)) != MXV_ERR_INVALID_ARG ||
        !strstr(mxv_policy_eval_last_error(), "mxv_policy_eval_categorical") || !strstr(mxv_ppo_last_error(), CB)) {
        ++bad;
        printf("BAD: the two headers' error slots are not separate: '%s' / '%s'\n", mxv_policy_eval_last_error(), mxv_ppo_last_error());
    }
    printf("ppo_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
