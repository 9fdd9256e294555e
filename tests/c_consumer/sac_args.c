/* The argument checks of the calls of include/mxv_sac.h driven from plain C: every call below must be refused with MXV_ERR_INVALID_ARG and
 * a message that names the call — in the header's own error slot, mxv_sac_last_error — before the device is touched (the addresses are
 * invented and never dereferenced).  Built by tests/test_sac_args_sanitized.py with AddressSanitizer + UBSan against the sanitized
 * library, so the host validation — the stride and range arithmetic at the 2^40 bound and at the top of the address space, the
 * alignment and overlap loops over up to ten inputs and four outputs, the thread-local error slot — runs instrumented. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "mxv_dqn.h"
#include "mxv_sac.h"

#define P(x) ((void *)(uintptr_t)(x))
#define U 0x1000000ull
#define ROWS 16
static int calls = 0, bad = 0;

/* q U, targets 2U, reward 3U, terminated 4U, next_q 5U, next_log_prob 6U, alpha_dev 7U, discount 8U, weights 9U, log_prob 10U, grad_loss 11U,
 * workspace 12U, td_error 13U, loss_out 14U, stats_out 15U, grad_q 16U, grad_log_prob 17U, targets_out 18U; a row is C = 2 critics */
typedef struct {
    int64_t M;
    int32_t C;
    void *q;
    int64_t q_ld;
    void *targets, *reward, *terminated, *next_q;
    int64_t next_ld;
    void *next_lp;
    double alpha;
    void *alpha_dev;
    double gamma;
    void *discount;
    double delta;
    void *weights, *log_prob, *grad_loss, *ws;
    int64_t ws_bytes;
    void *td, *loss, *stats, *grad_q, *grad_lp, *out;
} Args;

/* the bootstrap mode with everything optional present */
static Args boot(void) {
    Args a = {ROWS,     2,        P(U),     2,        NULL,      P(3 * U),  P(4 * U),  P(5 * U),  2,         P(6 * U),  0.2,       P(7 * U), 0.99,
              P(8 * U), 1.0,      P(9 * U), P(10 * U), P(11 * U), P(12 * U), 64,        P(13 * U), P(14 * U), P(15 * U), P(16 * U), P(17 * U), P(18 * U)};
    return a;
}

/* the targets mode */
static Args given(void) {
    Args a = boot();
    a.targets = P(2 * U);
    a.reward = a.terminated = a.next_q = a.next_lp = a.alpha_dev = a.discount = NULL;
    a.next_ld = 0;
    return a;
}

static int tgt(const Args *a) {
    return mxv_sac_targets(NULL, a->M, a->C, (const float *)a->next_q, a->next_ld, (const float *)a->reward, (const uint8_t *)a->terminated,
                           (const float *)a->next_lp, a->alpha, (const float *)a->alpha_dev, a->gamma, (const float *)a->discount, (float *)a->out);
}

static int fwd(const Args *a) {
    return mxv_sac_loss(NULL, a->M, a->C, (const float *)a->q, a->q_ld, (const float *)a->targets, (const float *)a->reward,
                        (const uint8_t *)a->terminated, (const float *)a->next_q, a->next_ld, (const float *)a->next_lp, a->alpha,
                        (const float *)a->alpha_dev, a->gamma, (const float *)a->discount, a->delta, (const float *)a->weights, a->ws, a->ws_bytes,
                        (float *)a->td, (float *)a->loss, (float *)a->stats);
}

static int bwd(const Args *a) {
    return mxv_sac_loss_backward(NULL, a->M, a->C, (const float *)a->q, a->q_ld, (const float *)a->targets, (const float *)a->reward,
                                 (const uint8_t *)a->terminated, (const float *)a->next_q, a->next_ld, (const float *)a->next_lp, a->alpha,
                                 (const float *)a->alpha_dev, a->gamma, (const float *)a->discount, a->delta, (const float *)a->weights,
                                 (const float *)a->grad_loss, (float *)a->grad_q);
}

static int pfwd(const Args *a) {
    return mxv_sac_policy_loss(NULL, a->M, a->C, (const float *)a->log_prob, (const float *)a->q, a->q_ld, a->alpha, (const float *)a->alpha_dev,
                               (const float *)a->weights, a->ws, a->ws_bytes, (float *)a->loss, (float *)a->stats);
}

static int pbwd(const Args *a) {
    return mxv_sac_policy_loss_backward(NULL, a->M, a->C, (const float *)a->log_prob, (const float *)a->q, a->q_ld, a->alpha,
                                        (const float *)a->alpha_dev, (const float *)a->weights, (const float *)a->grad_loss, (float *)a->grad_lp,
                                        (float *)a->grad_q);
}

static void expect(int rc, const char *api, const char *what) {
    const char *msg = mxv_sac_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what) || strncmp(msg, api, strlen(api)) != 0 || msg[strlen(api)] != ':') {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s: ... %s'\n", rc, msg ? msg : "(null)", api, what);
    }
}

#define ST "mxv_sac_targets"
#define SL "mxv_sac_loss"
#define SB "mxv_sac_loss_backward"
#define PL "mxv_sac_policy_loss"
#define PB "mxv_sac_policy_loss_backward"
/* one refused call: START from boot() or given(), EDIT the arguments, CALL one entry point */
#define REFUSE(START, EDIT, CALL, API, WHAT) \
    do {                                      \
        Args a = START();                     \
        EDIT;                                 \
        expect(CALL(&a), API, WHAT);          \
    } while (0)
/* the critics' forward and backward */
#define CRITICS(START, EDIT, WHAT)         \
    REFUSE(START, EDIT, fwd, SL, WHAT);    \
    REFUSE(START, EDIT, bwd, SB, WHAT)
/* the actor's forward and backward */
#define ACTOR(EDIT, WHAT)                  \
    REFUSE(boot, EDIT, pfwd, PL, WHAT);    \
    REFUSE(boot, EDIT, pbwd, PB, WHAT)
/* the four calls that read q */
#define LOSSES(EDIT, WHAT)     \
    CRITICS(boot, EDIT, WHAT); \
    ACTOR(EDIT, WHAT)
/* all five */
#define ALL(EDIT, WHAT)                 \
    REFUSE(boot, EDIT, tgt, ST, WHAT);  \
    LOSSES(EDIT, WHAT)

int main(void) {
    const int64_t big = (int64_t)1 << 40;
    const char *before = mxv_sac_last_error();
    ++calls;
    if (!before || before[0] != '\0') {
        ++bad;
        printf("BAD: the slot is not empty before the first call\n");
    }
    ++calls;
    if (mxv_sac_workspace_bytes(0) != 0 || mxv_sac_workspace_bytes(big + 1) != 0 || mxv_sac_workspace_bytes(ROWS) != 64 ||
        mxv_sac_workspace_bytes(1025) != 128 || mxv_sac_workspace_bytes(((int64_t)1 << 20) + 1) != (1025 + 2) * 64) {
        ++bad;
        printf("BAD: mxv_sac_workspace_bytes\n");
    }

    /* ---- NULL pointers, the sizes, the strides ---- */
    LOSSES(a.q = NULL, "q pointer is NULL");
    ACTOR(a.log_prob = NULL, "log_prob pointer is NULL");
    REFUSE(boot, a.next_q = NULL, tgt, ST, "next_q pointer is NULL");
    REFUSE(boot, a.reward = NULL, tgt, ST, "reward pointer is NULL");
    REFUSE(boot, a.terminated = NULL, tgt, ST, "terminated pointer is NULL");
    REFUSE(boot, a.out = NULL, tgt, ST, "targets_out pointer is NULL");
    ALL(a.M = 0, "M =");
    ALL(a.M = -3, "M =");
    ALL(a.M = INT64_MIN, "M =");
    ALL(a.M = big + 1, "2^40");
    ALL(a.M = INT64_MAX, "2^40");
    ALL(a.C = 0, "C =");
    ALL(a.C = -1, "C =");
    ALL(a.C = 65, "C =");
    LOSSES(a.q_ld = 1, "q_ld =");
    LOSSES(a.q_ld = -2, "q_ld =");
    LOSSES(a.C = 64; a.q_ld = 63; a.next_ld = 64, "q_ld =");
    LOSSES(a.q_ld = INT64_MAX, "beyond 2^40 elements");
    LOSSES(a.M = big; a.q_ld = 3; a.next_ld = 3, "beyond 2^40 elements");
    REFUSE(boot, a.next_ld = 1, tgt, ST, "next_q_ld =");
    REFUSE(boot, a.next_ld = INT64_MAX, tgt, ST, "beyond 2^40 elements");
    CRITICS(boot, a.next_ld = 1, "next_q_ld =");
    CRITICS(boot, a.next_ld = 0, "next_q_ld =");
    CRITICS(boot, a.next_ld = INT64_MAX, "beyond 2^40 elements");

    /* ---- exactly one target mode; what belongs to the bootstrap ---- */
    CRITICS(boot, a.targets = P(2 * U), "exactly one target mode");
    CRITICS(given, a.reward = P(3 * U), "exactly one target mode");
    CRITICS(given, a.targets = NULL, "exactly one target mode");
    CRITICS(given, a.discount = P(8 * U), "discount is given with targets");
    CRITICS(given, a.next_lp = P(6 * U), "next_log_prob is given with targets");
    CRITICS(given, a.alpha_dev = P(7 * U), "alpha_dev is given with targets");
    CRITICS(boot, a.reward = NULL, "reward pointer is NULL in the bootstrap mode");
    CRITICS(boot, a.terminated = NULL, "terminated pointer is NULL in the bootstrap mode");
    CRITICS(boot, a.next_q = NULL, "next_q pointer is NULL in the bootstrap mode");

    /* ---- the scalars: gamma is checked beside a discount too; alpha only where it is read; delta ---- */
    REFUSE(boot, a.gamma = INFINITY, tgt, ST, "gamma =");
    REFUSE(boot, a.gamma = NAN, tgt, ST, "gamma =");
    REFUSE(boot, a.discount = NULL; a.gamma = -INFINITY, tgt, ST, "gamma =");
    CRITICS(boot, a.gamma = INFINITY, "gamma =");
    CRITICS(boot, a.gamma = NAN, "gamma =");
    CRITICS(given, a.gamma = NAN, "gamma =");
    REFUSE(boot, a.next_lp = NULL, tgt, ST, "alpha_dev is given without next_log_prob");
    CRITICS(boot, a.next_lp = NULL, "alpha_dev is given without next_log_prob");
    REFUSE(boot, a.alpha_dev = NULL; a.alpha = NAN, tgt, ST, "alpha =");
    REFUSE(boot, a.alpha_dev = NULL; a.alpha = INFINITY, tgt, ST, "alpha =");
    CRITICS(boot, a.alpha_dev = NULL; a.alpha = NAN, "alpha =");
    ACTOR(a.alpha_dev = NULL; a.alpha = NAN, "alpha =");
    ACTOR(a.alpha_dev = NULL; a.alpha = -INFINITY, "alpha =");
    CRITICS(boot, a.delta = 0.0, "delta =");
    CRITICS(boot, a.delta = -1.0, "delta =");
    CRITICS(given, a.delta = NAN, "delta =");

    /* ---- the outputs and the workspace ---- */
    REFUSE(boot, a.loss = NULL, fwd, SL, "loss_out pointer is NULL");
    REFUSE(boot, a.stats = NULL, fwd, SL, "stats_out pointer is NULL");
    REFUSE(boot, a.ws = NULL, fwd, SL, "workspace pointer is NULL");
    REFUSE(boot, a.ws_bytes = 63, fwd, SL, "workspace_bytes =");
    REFUSE(boot, a.ws_bytes = -1, fwd, SL, "workspace_bytes =");
    REFUSE(boot, a.M = 1025; a.ws_bytes = 127, fwd, SL, "workspace_bytes =");
    REFUSE(boot, a.ws = P(12 * U + 4), fwd, SL, "workspace pointer");
    REFUSE(boot, a.loss = NULL, pfwd, PL, "loss_out pointer is NULL");
    REFUSE(boot, a.stats = NULL, pfwd, PL, "stats_out pointer is NULL");
    REFUSE(boot, a.ws = NULL, pfwd, PL, "workspace pointer is NULL");
    REFUSE(boot, a.ws_bytes = 63, pfwd, PL, "workspace_bytes =");
    REFUSE(boot, a.ws = P(12 * U + 4), pfwd, PL, "workspace pointer");
    REFUSE(boot, a.grad_loss = NULL, bwd, SB, "grad_loss pointer is NULL");
    REFUSE(boot, a.grad_q = NULL, bwd, SB, "grad_q pointer is NULL");
    REFUSE(boot, a.grad_loss = NULL, pbwd, PB, "grad_loss pointer is NULL");
    REFUSE(boot, a.grad_lp = NULL, pbwd, PB, "grad_log_prob pointer is NULL");
    REFUSE(boot, a.grad_q = NULL, pbwd, PB, "grad_q pointer is NULL");

    /* ---- alignment and the top of the address space ---- */
    LOSSES(a.q = P(U + 2), "q pointer");
    ACTOR(a.log_prob = P(10 * U + 1), "log_prob pointer");
    ALL(a.alpha_dev = P(7 * U + 2), "alpha_dev pointer");
    LOSSES(a.weights = P(9 * U + 3), "weights pointer");
    CRITICS(given, a.targets = P(2 * U + 2), "targets pointer");
    CRITICS(boot, a.reward = P(3 * U + 1), "reward pointer");
    CRITICS(boot, a.next_q = P(5 * U + 2), "next_q pointer");
    CRITICS(boot, a.next_lp = P(6 * U + 2), "next_log_prob pointer");
    CRITICS(boot, a.discount = P(8 * U + 2), "discount pointer");
    REFUSE(boot, a.next_q = P(5 * U + 2), tgt, ST, "next_q pointer");
    REFUSE(boot, a.next_lp = P(6 * U + 1), tgt, ST, "next_log_prob pointer");
    REFUSE(boot, a.discount = P(8 * U + 3), tgt, ST, "discount pointer");
    REFUSE(boot, a.out = P(18 * U + 2), tgt, ST, "targets_out pointer");
    REFUSE(boot, a.td = P(13 * U + 2), fwd, SL, "td_error pointer");
    REFUSE(boot, a.loss = P(14 * U + 1), fwd, SL, "loss_out pointer");
    REFUSE(boot, a.stats = P(15 * U + 2), pfwd, PL, "stats_out pointer");
    REFUSE(boot, a.grad_loss = P(11 * U + 2), bwd, SB, "grad_loss pointer");
    REFUSE(boot, a.grad_q = P(16 * U + 2), bwd, SB, "grad_q pointer");
    REFUSE(boot, a.grad_lp = P(17 * U + 2), pbwd, PB, "grad_log_prob pointer");
    LOSSES(a.q = P(UINTPTR_MAX - 15), "address space");
    ALL(a.alpha_dev = P(UINTPTR_MAX - 3), "address space");
    LOSSES(a.weights = P(UINTPTR_MAX - 31), "address space");
    ACTOR(a.log_prob = P(UINTPTR_MAX - 15), "address space");
    CRITICS(boot, a.terminated = P(UINTPTR_MAX - 3), "address space");
    CRITICS(boot, a.next_q = P(UINTPTR_MAX - 15), "address space");
    CRITICS(boot, a.next_lp = P(UINTPTR_MAX - 31), "address space");
    CRITICS(boot, a.discount = P(UINTPTR_MAX - 31), "address space");
    REFUSE(boot, a.next_q = P(UINTPTR_MAX - 15), tgt, ST, "address space");
    REFUSE(boot, a.terminated = P(UINTPTR_MAX - 3), tgt, ST, "address space");
    REFUSE(boot, a.out = P(UINTPTR_MAX - 15), tgt, ST, "address space");
    REFUSE(boot, a.td = P(UINTPTR_MAX - 15), fwd, SL, "address space");
    REFUSE(boot, a.grad_q = P(UINTPTR_MAX - 63), bwd, SB, "address space");
    REFUSE(boot, a.grad_lp = P(UINTPTR_MAX - 31), pbwd, PB, "address space");

    /* ---- an output shares a byte with an input or with another output ---- */
    REFUSE(boot, a.out = P(5 * U + 124), tgt, ST, "targets_out overlaps the next_q");
    REFUSE(boot, a.next_ld = 5; a.out = P(5 * U + 15 * 20 + 4), tgt, ST, "targets_out overlaps the next_q"); /* the last strided row */
    REFUSE(boot, a.out = P(3 * U + 60), tgt, ST, "targets_out overlaps the reward");
    REFUSE(boot, a.out = P(4 * U + 12), tgt, ST, "targets_out overlaps the terminated");
    REFUSE(boot, a.out = P(6 * U - 60), tgt, ST, "targets_out overlaps the next_log_prob");
    REFUSE(boot, a.out = P(7 * U), tgt, ST, "targets_out overlaps alpha_dev");
    REFUSE(boot, a.out = P(8 * U + 60), tgt, ST, "targets_out overlaps the discount");
    REFUSE(boot, a.td = P(U + 124), fwd, SL, "td_error overlaps the q");
    REFUSE(given, a.td = P(2 * U + 60), fwd, SL, "td_error overlaps the targets");
    REFUSE(boot, a.td = P(5 * U - 60), fwd, SL, "td_error overlaps the next_q");
    REFUSE(boot, a.loss = P(7 * U), fwd, SL, "loss_out overlaps alpha_dev");
    REFUSE(boot, a.stats = P(9 * U - 28), fwd, SL, "stats_out overlaps the weights");
    REFUSE(boot, a.stats = P(6 * U + 60), fwd, SL, "stats_out overlaps the next_log_prob");
    REFUSE(boot, a.ws = P(8 * U + 56), fwd, SL, "workspace overlaps the discount");
    REFUSE(boot, a.ws = P(3 * U - 56), fwd, SL, "workspace overlaps the reward");
    REFUSE(boot, a.td = P(12 * U + 60), fwd, SL, "outputs workspace and td_error overlap");
    REFUSE(boot, a.loss = P(13 * U + 60), fwd, SL, "outputs td_error and loss_out overlap");
    REFUSE(boot, a.stats = P(14 * U - 28), fwd, SL, "outputs loss_out and stats_out overlap");
    REFUSE(boot, a.grad_q = P(U + 124), bwd, SB, "grad_q overlaps the q");
    REFUSE(boot, a.grad_q = P(11 * U - 124), bwd, SB, "grad_q overlaps the grad_loss");
    REFUSE(boot, a.grad_q = P(4 * U + 15), bwd, SB, "grad_q pointer");
    REFUSE(boot, a.grad_q = P(4 * U + 12), bwd, SB, "grad_q overlaps the terminated");
    REFUSE(boot, a.loss = P(10 * U + 60), pfwd, PL, "loss_out overlaps the log_prob");
    REFUSE(boot, a.stats = P(U + 124), pfwd, PL, "stats_out overlaps the q");
    REFUSE(boot, a.ws = P(9 * U + 56), pfwd, PL, "workspace overlaps the weights");
    REFUSE(boot, a.stats = P(12 * U + 60), pfwd, PL, "outputs workspace and stats_out overlap");
    REFUSE(boot, a.grad_lp = P(10 * U + 60), pbwd, PB, "grad_log_prob overlaps the log_prob");
    REFUSE(boot, a.grad_q = P(7 * U - 124), pbwd, PB, "grad_q overlaps alpha_dev");
    REFUSE(boot, a.grad_lp = P(11 * U), pbwd, PB, "grad_log_prob overlaps the grad_loss");
    REFUSE(boot, a.grad_q = P(17 * U + 60), pbwd, PB, "outputs grad_log_prob and grad_q overlap");
    REFUSE(boot, a.grad_lp = P(16 * U + 124), pbwd, PB, "outputs grad_log_prob and grad_q overlap");

    /* the slot is this header's own: a refusal of a Q-learning-loss call lands in mxv_dqn_last_error and leaves this one alone */
    ++calls;
    if (mxv_dqn_workspace_bytes(ROWS) != mxv_sac_workspace_bytes(ROWS) ||
        mxv_dqn_loss_backward(NULL, 0, 2, (const float *)P(U), 2, P(2 * U), 8, (const float *)P(3 * U), NULL, NULL, NULL, 0, NULL, 0, 0.99, 1.0, NULL,
                              (const float *)P(4 * U), (float *)P(5 * U)) != MXV_ERR_INVALID_ARG ||
        !strstr(mxv_dqn_last_error(), "mxv_dqn_loss_backward") || !strstr(mxv_sac_last_error(), PB) || strstr(mxv_sac_last_error(), "mxv_dqn")) {
        ++bad;
        printf("BAD: the two headers' error slots are not separate: '%s' / '%s'\n", mxv_dqn_last_error(), mxv_sac_last_error());
    }
    printf("sac_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
