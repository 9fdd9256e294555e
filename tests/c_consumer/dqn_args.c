/* The argument checks of the calls of include/mxv_dqn.h driven from plain C: every call below must be refused with MXV_ERR_INVALID_ARG and
 * a message that names the call — in the header's own error slot, mxv_dqn_last_error — before the device is touched (the addresses are
 * invented and never dereferenced).  Built by tests/test_dqn_args_sanitized.py with AddressSanitizer + UBSan against the sanitized
 * library, so the host validation — the workspace arithmetic at the 2^40 bound, the stride and range arithmetic at the top of the
 * address space, the alignment and overlap loops over nine inputs and four outputs, the thread-local error slot — runs instrumented. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "mxv_dqn.h"
#include "mxv_ppo.h"

#define P(x) ((void *)(uintptr_t)(x))
#define U 0x1000000ull
#define WS 64 /* mxv_dqn_workspace_bytes of up to 1024 rows */
static int calls = 0, bad = 0;

/* q U, actions 2U, targets 3U, reward 4U, terminated 5U, next_q 6U, next_q_online 7U, weights 8U; forward: workspace 9U, td_error 10U,
 * loss 11U, stats 12U; backward: grad_loss 9U, grad_q 10U */
typedef struct {
    int64_t M;
    int32_t A;
    void *q;
    int64_t q_ld;
    void *actions;
    int32_t action_bytes;
    void *targets, *reward, *terminated, *next_q;
    int64_t next_q_ld;
    void *online;
    int64_t online_ld;
    double gamma, delta;
    void *weights;
    void *workspace;
    int64_t workspace_bytes;
    void *td_error, *loss, *stats; /* forward */
    void *grad_loss, *grad_q;      /* backward */
} Args;

static Args bootstrap(void) {
    Args a = {16, 4, P(U), 4, P(2 * U), 8, NULL, P(4 * U), P(5 * U), P(6 * U), 4, P(7 * U), 4, 0.99, 1.0, P(8 * U),
              P(9 * U), WS, P(10 * U), P(11 * U), P(12 * U), P(9 * U), P(10 * U)};
    return a;
}

static Args with_targets(void) {
    Args a = bootstrap();
    a.targets = P(3 * U);
    a.reward = a.terminated = a.next_q = a.online = NULL;
    return a;
}

static int fwd(const Args *a) {
    return mxv_dqn_loss(NULL, a->M, a->A, (const float *)a->q, a->q_ld, a->actions, a->action_bytes, (const float *)a->targets, (const float *)a->reward,
                        (const uint8_t *)a->terminated, (const float *)a->next_q, a->next_q_ld, (const float *)a->online, a->online_ld, a->gamma,
                        a->delta, (const float *)a->weights, a->workspace, a->workspace_bytes, (float *)a->td_error, (float *)a->loss, (float *)a->stats);
}

static int bwd(const Args *a) {
    return mxv_dqn_loss_backward(NULL, a->M, a->A, (const float *)a->q, a->q_ld, a->actions, a->action_bytes, (const float *)a->targets,
                                 (const float *)a->reward, (const uint8_t *)a->terminated, (const float *)a->next_q, a->next_q_ld,
                                 (const float *)a->online, a->online_ld, a->gamma, a->delta, (const float *)a->weights, (const float *)a->grad_loss,
                                 (float *)a->grad_q);
}

static void expect(int rc, const char *api, const char *what) {
    const char *msg = mxv_dqn_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what) || strncmp(msg, api, strlen(api)) != 0 || msg[strlen(api)] != ':') {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s: ... %s'\n", rc, msg ? msg : "(null)", api, what);
    }
}

#define DL "mxv_dqn_loss"
#define DB "mxv_dqn_loss_backward"
/* one refused call: START from bootstrap() or with_targets(), EDIT the arguments, CALL fwd or bwd */
#define REFUSE(START, EDIT, CALL, API, WHAT) \
    do {                                      \
        Args a = START();                     \
        EDIT;                                 \
        expect(CALL(&a), API, WHAT);          \
    } while (0)
/* what both entry points check alike */
#define BOTH(START, EDIT, WHAT)              \
    REFUSE(START, EDIT, fwd, DL, WHAT);      \
    REFUSE(START, EDIT, bwd, DB, WHAT)

int main(void) {
    const int64_t big = (int64_t)1 << 40;
    const char *before = mxv_dqn_last_error();
    ++calls;
    if (!before || before[0] != '\0') {
        ++bad;
        printf("BAD: the slot is not empty before the first call\n");
    }

    /* ---- the workspace size: no status, 0 outside 1..2^40 ---- */
    ++calls;
    if (mxv_dqn_workspace_bytes(0) != 0 || mxv_dqn_workspace_bytes(-5) != 0 || mxv_dqn_workspace_bytes(INT64_MIN) != 0 ||
        mxv_dqn_workspace_bytes(big + 1) != 0 || mxv_dqn_workspace_bytes(INT64_MAX) != 0 || mxv_dqn_workspace_bytes(1) != WS ||
        mxv_dqn_workspace_bytes(1024) != WS || mxv_dqn_workspace_bytes(1025) != 2 * WS || mxv_dqn_workspace_bytes(1 << 20) != 1024 * WS ||
        mxv_dqn_workspace_bytes((1 << 20) + 1) != (1025 + 2) * WS || mxv_dqn_workspace_bytes(big) != (((int64_t)1 << 30) + (1 << 20) + 1024) * WS) {
        ++bad;
        printf("BAD: mxv_dqn_workspace_bytes\n");
    }

    /* ---- NULL pointers, the sizes, the strides, the action width ---- */
    BOTH(bootstrap, a.q = NULL, "q pointer is NULL");
    BOTH(bootstrap, a.actions = NULL, "actions pointer is NULL");
    BOTH(bootstrap, a.M = 0, "M =");
    BOTH(bootstrap, a.M = -3, "M =");
    BOTH(bootstrap, a.M = INT64_MIN, "M =");
    BOTH(bootstrap, a.M = big + 1; a.workspace_bytes = INT64_MAX, "2^40");
    BOTH(bootstrap, a.M = INT64_MAX; a.workspace_bytes = INT64_MAX, "2^40");
    BOTH(bootstrap, a.A = 0, "A =");
    BOTH(bootstrap, a.A = -1, "A =");
    BOTH(bootstrap, a.A = 65, "A =");
    BOTH(bootstrap, a.q_ld = 3, "q_ld =");
    BOTH(bootstrap, a.q_ld = -4, "q_ld =");
    BOTH(bootstrap, a.q_ld = INT64_MAX, "beyond 2^40 elements");
    BOTH(bootstrap, a.M = big; a.q_ld = 5; a.workspace_bytes = INT64_MAX, "beyond 2^40 elements");
    BOTH(bootstrap, a.next_q_ld = 3, "next_q_ld =");
    BOTH(bootstrap, a.next_q_ld = INT64_MAX, "beyond 2^40 elements");
    BOTH(bootstrap, a.online_ld = 0, "next_q_online_ld =");
    BOTH(bootstrap, a.online_ld = INT64_MAX, "beyond 2^40 elements");
    BOTH(bootstrap, a.action_bytes = 0, "action_bytes =");
    BOTH(bootstrap, a.action_bytes = 2, "action_bytes =");
    BOTH(bootstrap, a.action_bytes = 16, "action_bytes =");

    /* ---- exactly one target mode ---- */
    BOTH(bootstrap, a.targets = P(3 * U), "exactly one target mode");
    BOTH(with_targets, a.reward = P(4 * U), "exactly one target mode");
    BOTH(with_targets, a.terminated = P(5 * U), "exactly one target mode");
    BOTH(with_targets, a.next_q = P(6 * U), "exactly one target mode");
    BOTH(with_targets, a.targets = NULL, "exactly one target mode");
    BOTH(with_targets, a.online = P(7 * U), "next_q_online is given with targets");
    BOTH(bootstrap, a.reward = NULL, "reward pointer is NULL");
    BOTH(bootstrap, a.terminated = NULL, "terminated pointer is NULL");
    BOTH(bootstrap, a.next_q = NULL, "next_q pointer is NULL");

    /* ---- the scalars ---- */
    BOTH(bootstrap, a.gamma = INFINITY, "gamma =");
    BOTH(bootstrap, a.gamma = -INFINITY, "gamma =");
    BOTH(bootstrap, a.gamma = NAN, "gamma =");
    BOTH(with_targets, a.gamma = NAN, "gamma =");
    BOTH(bootstrap, a.delta = 0.0, "delta =");
    BOTH(bootstrap, a.delta = -0.5, "delta =");
    BOTH(bootstrap, a.delta = NAN, "delta =");
    BOTH(bootstrap, a.delta = -INFINITY, "delta =");

    /* ---- alignment and the top of the address space: the inputs ---- */
    BOTH(bootstrap, a.q = P(U + 2), "q pointer");
    BOTH(bootstrap, a.actions = P(2 * U + 4), "actions pointer");
    BOTH(bootstrap, a.action_bytes = 4; a.actions = P(2 * U + 2), "actions pointer");
    BOTH(with_targets, a.targets = P(3 * U + 1), "targets pointer");
    BOTH(bootstrap, a.reward = P(4 * U + 3), "reward pointer");
    BOTH(bootstrap, a.next_q = P(6 * U + 2), "next_q pointer");
    BOTH(bootstrap, a.online = P(7 * U + 1), "next_q_online pointer");
    BOTH(bootstrap, a.weights = P(8 * U + 2), "weights pointer");
    BOTH(bootstrap, a.q = P(UINTPTR_MAX - 15), "address space");
    BOTH(bootstrap, a.actions = P(UINTPTR_MAX - 7), "address space");
    BOTH(bootstrap, a.terminated = P(UINTPTR_MAX - 3), "address space");
    BOTH(bootstrap, a.next_q = P(UINTPTR_MAX - 63), "address space");
    BOTH(bootstrap, a.online = P(UINTPTR_MAX - 63), "address space");
    BOTH(bootstrap, a.weights = P(UINTPTR_MAX - 15), "address space");

    /* ---- the forward's own ---- */
    REFUSE(bootstrap, a.workspace = NULL, fwd, DL, "workspace pointer is NULL");
    REFUSE(bootstrap, a.loss = NULL, fwd, DL, "loss_out pointer is NULL");
    REFUSE(bootstrap, a.stats = NULL, fwd, DL, "stats_out pointer is NULL");
    REFUSE(bootstrap, a.workspace_bytes = WS - 1, fwd, DL, "workspace_bytes =");
    REFUSE(bootstrap, a.workspace_bytes = 0, fwd, DL, "workspace_bytes =");
    REFUSE(bootstrap, a.workspace_bytes = -WS, fwd, DL, "workspace_bytes =");
    REFUSE(bootstrap, a.M = 1025, fwd, DL, "workspace_bytes =");
    REFUSE(with_targets, a.M = 1 << 20; a.workspace_bytes = 1023 * WS, fwd, DL, "workspace_bytes =");
    REFUSE(bootstrap, a.workspace = P(9 * U + 4), fwd, DL, "workspace pointer");
    REFUSE(bootstrap, a.td_error = P(10 * U + 2), fwd, DL, "td_error pointer");
    REFUSE(bootstrap, a.loss = P(11 * U + 1), fwd, DL, "loss_out pointer");
    REFUSE(bootstrap, a.stats = P(12 * U + 3), fwd, DL, "stats_out pointer");
    REFUSE(bootstrap, a.workspace = P(UINTPTR_MAX - 15), fwd, DL, "address space");
    REFUSE(bootstrap, a.td_error = P(UINTPTR_MAX - 31), fwd, DL, "address space");
    REFUSE(bootstrap, a.stats = P(UINTPTR_MAX - 15), fwd, DL, "address space");
    REFUSE(bootstrap, a.workspace = P(U + 8), fwd, DL, "workspace overlaps the q");
    REFUSE(bootstrap, a.workspace = P(2 * U - 56), fwd, DL, "workspace overlaps the actions");
    REFUSE(with_targets, a.td_error = P(3 * U + 60), fwd, DL, "td_error overlaps the targets");
    REFUSE(bootstrap, a.td_error = P(4 * U - 60), fwd, DL, "td_error overlaps the reward");
    REFUSE(bootstrap, a.td_error = P(5 * U + 12), fwd, DL, "td_error overlaps the terminated");
    REFUSE(bootstrap, a.loss = P(6 * U + 252), fwd, DL, "loss_out overlaps the next_q");
    REFUSE(bootstrap, a.stats = P(7 * U - 4), fwd, DL, "stats_out overlaps the next_q_online");
    REFUSE(bootstrap, a.loss = P(8 * U), fwd, DL, "loss_out overlaps the weights");
    REFUSE(bootstrap, a.q_ld = 9; a.stats = P(U + 15 * 36), fwd, DL, "stats_out overlaps the q"); /* the last strided row */
    REFUSE(bootstrap, a.td_error = P(9 * U + 60), fwd, DL, "outputs workspace and td_error overlap");
    REFUSE(bootstrap, a.loss = P(9 * U + 32), fwd, DL, "outputs workspace and loss_out overlap");
    REFUSE(bootstrap, a.loss = P(10 * U + 60), fwd, DL, "outputs td_error and loss_out overlap");
    REFUSE(bootstrap, a.stats = P(10 * U - 4), fwd, DL, "outputs td_error and stats_out overlap");
    REFUSE(bootstrap, a.stats = P(11 * U - 28), fwd, DL, "outputs loss_out and stats_out overlap");

    /* ---- the backward's own ---- */
    REFUSE(bootstrap, a.grad_loss = NULL, bwd, DB, "grad_loss pointer is NULL");
    REFUSE(bootstrap, a.grad_q = NULL, bwd, DB, "grad_q pointer is NULL");
    REFUSE(bootstrap, a.grad_loss = P(9 * U + 2), bwd, DB, "grad_loss pointer");
    REFUSE(bootstrap, a.grad_q = P(10 * U + 1), bwd, DB, "grad_q pointer");
    REFUSE(bootstrap, a.grad_loss = P(UINTPTR_MAX - 3), bwd, DB, "address space");
    REFUSE(bootstrap, a.grad_q = P(UINTPTR_MAX - 63), bwd, DB, "address space");
    REFUSE(bootstrap, a.grad_q = P(U + 252), bwd, DB, "grad_q overlaps the q");
    REFUSE(bootstrap, a.grad_q = P(2 * U - 252), bwd, DB, "grad_q overlaps the actions");
    REFUSE(with_targets, a.grad_q = P(3 * U + 60), bwd, DB, "grad_q overlaps the targets");
    REFUSE(bootstrap, a.grad_q = P(6 * U - 4), bwd, DB, "grad_q overlaps the next_q");
    REFUSE(bootstrap, a.grad_q = P(8 * U + 60), bwd, DB, "grad_q overlaps the weights");
    REFUSE(bootstrap, a.grad_q = P(9 * U - 252), bwd, DB, "grad_q overlaps the grad_loss");

    /* delta = +Inf is the half squared error, not an error: the call gets as far as the next check */
    REFUSE(bootstrap, a.delta = INFINITY; a.loss = NULL, fwd, DL, "loss_out pointer is NULL");
    REFUSE(bootstrap, a.delta = INFINITY; a.grad_q = NULL, bwd, DB, "grad_q pointer is NULL");

    /* the slot is this header's own: a refusal of a PPO call lands in mxv_ppo_last_error and leaves this one alone */
    ++calls;
    if (mxv_ppo_advantage_moments(NULL, 0, (const float *)P(U), 1e-8, P(2 * U), 64, (double *)P(3 * U)) != MXV_ERR_INVALID_ARG ||
        !strstr(mxv_ppo_last_error(), "mxv_ppo_advantage_moments") || !strstr(mxv_dqn_last_error(), DB)) {
        ++bad;
        printf("BAD: the two headers' error slots are not separate: '%s' / '%s'\n", mxv_ppo_last_error(), mxv_dqn_last_error());
    }
    printf("dqn_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
