/* The argument checks of the calls of include/mxv_qr.h driven from plain C: every call below must be refused with MXV_ERR_INVALID_ARG and
 * a message that names the call — in the header's own error slot, mxv_qr_last_error — before the device is touched (the addresses are
 * invented and never dereferenced).  Built by tests/test_qr_args_sanitized.py with AddressSanitizer + UBSan against the sanitized
 * library, so the host validation — the workspace arithmetic at the 2^40 bound, the stride and range arithmetic at the top of the
 * address space, the alignment and overlap loops over ten inputs and five outputs, the thread-local error slot — runs instrumented.
 * Every refusal the header lists is made once, through each entry point that makes it. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "mxv_qr.h"
#include "mxv_c51.h"

#define P(x) ((void *)(uintptr_t)(x))
#define U 0x1000000ull
#define ROWS 16
#define WS (48 * ROWS + 64) /* mxv_qr_workspace_bytes of 16 rows: six doubles a row and one leaf */
static int calls = 0, bad = 0;

/* quantiles U, actions 2U, target_quantiles 3U, reward 4U, terminated 5U, next_quantiles 6U, next_quantiles_online 7U, weights 8U,
 * discount 14U; forward: workspace 9U, row_loss 10U, targets_out 11U, loss 12U, stats 13U; backward: grad_loss 9U, grad_quantiles 10U;
 * q_values: q_out 9U */
typedef struct {
    int64_t M;
    int32_t A, N;
    void *quantiles;
    int64_t ld;
    void *actions;
    int32_t action_bytes;
    void *target_quantiles, *reward, *terminated, *next;
    int64_t next_ld;
    void *online;
    int64_t online_ld;
    double gamma;
    void *discount;
    double kappa;
    void *weights;
    void *workspace;
    int64_t workspace_bytes;
    void *row_loss, *targets_out, *loss, *stats; /* forward */
    void *grad_loss, *grad;                      /* backward */
    void *q_out;                                 /* q_values */
} Args;

static Args bootstrap(void) {
    Args a = {ROWS, 4, 5, P(U), 20, P(2 * U), 8, NULL, P(4 * U), P(5 * U), P(6 * U), 20, P(7 * U), 20, 0.99, P(14 * U), 1.0, P(8 * U),
              P(9 * U), WS, P(10 * U), P(11 * U), P(12 * U), P(13 * U), P(9 * U), P(10 * U), P(9 * U)};
    return a;
}

static Args given(void) {
    Args a = bootstrap();
    a.target_quantiles = P(3 * U);
    a.reward = a.terminated = a.next = a.online = a.discount = NULL;
    return a;
}

static int fwd(const Args *a) {
    return mxv_qr_loss(NULL, a->M, a->A, a->N, (const float *)a->quantiles, a->ld, a->actions, a->action_bytes, (const float *)a->target_quantiles,
                       (const float *)a->reward, (const uint8_t *)a->terminated, (const float *)a->next, a->next_ld, (const float *)a->online,
                       a->online_ld, a->gamma, (const float *)a->discount, a->kappa, (const float *)a->weights, a->workspace, a->workspace_bytes,
                       (float *)a->row_loss, (float *)a->targets_out, (float *)a->loss, (float *)a->stats);
}

static int bwd(const Args *a) {
    return mxv_qr_loss_backward(NULL, a->M, a->A, a->N, (const float *)a->quantiles, a->ld, a->actions, a->action_bytes,
                                (const float *)a->target_quantiles, (const float *)a->reward, (const uint8_t *)a->terminated, (const float *)a->next,
                                a->next_ld, (const float *)a->online, a->online_ld, a->gamma, (const float *)a->discount, a->kappa,
                                (const float *)a->weights, (const float *)a->grad_loss, (float *)a->grad);
}

static int qv(const Args *a) { return mxv_qr_q_values(NULL, a->M, a->A, a->N, (const float *)a->quantiles, a->ld, (float *)a->q_out); }

static void expect(int rc, const char *api, const char *what) {
    const char *msg = mxv_qr_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what) || strncmp(msg, api, strlen(api)) != 0 || msg[strlen(api)] != ':') {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s: ... %s'\n", rc, msg ? msg : "(null)", api, what);
    }
}

#define QL "mxv_qr_loss"
#define QB "mxv_qr_loss_backward"
#define QQ "mxv_qr_q_values"
/* one refused call: START from bootstrap() or given(), EDIT the arguments, CALL fwd, bwd or qv */
#define REFUSE(START, EDIT, CALL, API, WHAT) \
    do {                                      \
        Args a = START();                     \
        EDIT;                                 \
        expect(CALL(&a), API, WHAT);          \
    } while (0)
/* what the loss and its backward check alike */
#define BOTH(START, EDIT, WHAT)              \
    REFUSE(START, EDIT, fwd, QL, WHAT);      \
    REFUSE(START, EDIT, bwd, QB, WHAT)
/* ... and the expected values too */
#define ALL(EDIT, WHAT)           \
    BOTH(bootstrap, EDIT, WHAT);  \
    REFUSE(bootstrap, EDIT, qv, QQ, WHAT)

int main(void) {
    const int64_t big = (int64_t)1 << 40;
    const char *before = mxv_qr_last_error();
    ++calls;
    if (!before || before[0] != '\0') {
        ++bad;
        printf("BAD: the slot is not empty before the first call\n");
    }

    /* ---- the workspace size: no status, 0 outside 1..2^40 ---- */
    ++calls;
    if (mxv_qr_workspace_bytes(0) != 0 || mxv_qr_workspace_bytes(-5) != 0 || mxv_qr_workspace_bytes(INT64_MIN) != 0 ||
        mxv_qr_workspace_bytes(big + 1) != 0 || mxv_qr_workspace_bytes(INT64_MAX) != 0 || mxv_qr_workspace_bytes(1) != 48 + 64 ||
        mxv_qr_workspace_bytes(ROWS) != WS || mxv_qr_workspace_bytes(1024) != 48 * 1024 + 64 || mxv_qr_workspace_bytes(1025) != 48 * 1025 + 128 ||
        mxv_qr_workspace_bytes(1 << 20) != 48 * (1 << 20) + 1024 * 64 || mxv_qr_workspace_bytes((1 << 20) + 1) != 48 * ((1 << 20) + 1) + (1025 + 2) * 64 ||
        mxv_qr_workspace_bytes(big) != 48 * big + (((int64_t)1 << 30) + (1 << 20) + 1024) * 64) {
        ++bad;
        printf("BAD: mxv_qr_workspace_bytes\n");
    }

    /* ---- NULL pointers, the sizes, kappa, the strides, the action width ---- */
    ALL(a.quantiles = NULL, "quantiles pointer is NULL");
    BOTH(bootstrap, a.actions = NULL, "actions pointer is NULL");
    ALL(a.M = 0, "M =");
    ALL(a.M = -3, "M =");
    ALL(a.M = INT64_MIN, "M =");
    ALL(a.M = big + 1; a.workspace_bytes = INT64_MAX, "2^40");
    ALL(a.M = INT64_MAX; a.workspace_bytes = INT64_MAX, "2^40");
    ALL(a.A = 0, "A =");
    ALL(a.A = -1, "A =");
    ALL(a.A = 65, "A =");
    ALL(a.N = 0, "N =");
    ALL(a.N = -7, "N =");
    ALL(a.N = 65, "N =");
    BOTH(bootstrap, a.kappa = 0.0, "kappa =");
    BOTH(bootstrap, a.kappa = -0.0, "kappa =");
    BOTH(bootstrap, a.kappa = -1.0, "kappa =");
    BOTH(bootstrap, a.kappa = INFINITY, "kappa =");
    BOTH(given, a.kappa = NAN, "kappa =");
    ALL(a.ld = 19, "quantiles_ld =");
    ALL(a.ld = -20, "quantiles_ld =");
    ALL(a.A = 64; a.N = 64; a.ld = 4095, "quantiles_ld =");
    ALL(a.ld = INT64_MAX, "beyond 2^40 elements");
    ALL(a.M = big; a.ld = 21; a.workspace_bytes = INT64_MAX, "beyond 2^40 elements");
    BOTH(bootstrap, a.next_ld = 19, "next_quantiles_ld =");
    BOTH(bootstrap, a.next_ld = INT64_MAX, "beyond 2^40 elements");
    BOTH(bootstrap, a.online_ld = 0, "next_quantiles_online_ld =");
    BOTH(bootstrap, a.online_ld = INT64_MAX, "beyond 2^40 elements");
    BOTH(bootstrap, a.action_bytes = 0, "action_bytes =");
    BOTH(bootstrap, a.action_bytes = 2, "action_bytes =");
    BOTH(bootstrap, a.action_bytes = 16, "action_bytes =");

    /* ---- exactly one target mode; what belongs to the bootstrap mode alone ---- */
    BOTH(bootstrap, a.target_quantiles = P(3 * U), "exactly one target mode");
    BOTH(given, a.reward = P(4 * U), "exactly one target mode");
    BOTH(given, a.terminated = P(5 * U), "exactly one target mode");
    BOTH(given, a.next = P(6 * U), "exactly one target mode");
    BOTH(given, a.target_quantiles = NULL, "exactly one target mode");
    BOTH(given, a.online = P(7 * U), "next_quantiles_online is given with target_quantiles");
    BOTH(given, a.discount = P(14 * U), "discount is given with target_quantiles");
    BOTH(bootstrap, a.reward = NULL, "reward pointer is NULL");
    BOTH(bootstrap, a.terminated = NULL, "terminated pointer is NULL");
    BOTH(bootstrap, a.next = NULL, "next_quantiles pointer is NULL");

    /* ---- the scalars ---- */
    BOTH(bootstrap, a.gamma = INFINITY, "gamma =");
    BOTH(bootstrap, a.gamma = -INFINITY, "gamma =");
    BOTH(bootstrap, a.gamma = NAN, "gamma =");
    BOTH(given, a.gamma = NAN, "gamma =");

    /* ---- alignment and the top of the address space: the inputs ---- */
    ALL(a.quantiles = P(U + 2), "quantiles pointer");
    BOTH(bootstrap, a.actions = P(2 * U + 4), "actions pointer");
    BOTH(bootstrap, a.action_bytes = 4; a.actions = P(2 * U + 2), "actions pointer");
    BOTH(given, a.target_quantiles = P(3 * U + 1), "target_quantiles pointer");
    BOTH(bootstrap, a.reward = P(4 * U + 3), "reward pointer");
    BOTH(bootstrap, a.next = P(6 * U + 2), "next_quantiles pointer");
    BOTH(bootstrap, a.online = P(7 * U + 1), "next_quantiles_online pointer");
    BOTH(bootstrap, a.discount = P(14 * U + 2), "discount pointer");
    BOTH(bootstrap, a.weights = P(8 * U + 2), "weights pointer");
    ALL(a.quantiles = P(UINTPTR_MAX - 15), "address space");
    BOTH(bootstrap, a.actions = P(UINTPTR_MAX - 7), "address space");
    BOTH(given, a.target_quantiles = P(UINTPTR_MAX - 63), "address space");
    BOTH(bootstrap, a.terminated = P(UINTPTR_MAX - 3), "address space");
    BOTH(bootstrap, a.next = P(UINTPTR_MAX - 63), "address space");
    BOTH(bootstrap, a.online = P(UINTPTR_MAX - 63), "address space");
    BOTH(bootstrap, a.discount = P(UINTPTR_MAX - 15), "address space");
    BOTH(bootstrap, a.weights = P(UINTPTR_MAX - 15), "address space");

    /* ---- the forward's own ---- */
    REFUSE(bootstrap, a.workspace = NULL, fwd, QL, "workspace pointer is NULL");
    REFUSE(bootstrap, a.loss = NULL, fwd, QL, "loss_out pointer is NULL");
    REFUSE(bootstrap, a.stats = NULL, fwd, QL, "stats_out pointer is NULL");
    REFUSE(bootstrap, a.workspace_bytes = WS - 1, fwd, QL, "workspace_bytes =");
    REFUSE(bootstrap, a.workspace_bytes = 0, fwd, QL, "workspace_bytes =");
    REFUSE(bootstrap, a.workspace_bytes = -WS, fwd, QL, "workspace_bytes =");
    REFUSE(bootstrap, a.M = ROWS + 1, fwd, QL, "workspace_bytes =");
    REFUSE(given, a.M = 1 << 20; a.workspace_bytes = 48 * (1 << 20) + 1023 * 64, fwd, QL, "workspace_bytes =");
    REFUSE(bootstrap, a.workspace = P(9 * U + 4), fwd, QL, "workspace pointer");
    REFUSE(bootstrap, a.row_loss = P(10 * U + 2), fwd, QL, "row_loss pointer");
    REFUSE(bootstrap, a.targets_out = P(11 * U + 2), fwd, QL, "targets_out pointer");
    REFUSE(bootstrap, a.loss = P(12 * U + 1), fwd, QL, "loss_out pointer");
    REFUSE(bootstrap, a.stats = P(13 * U + 3), fwd, QL, "stats_out pointer");
    REFUSE(bootstrap, a.workspace = P(UINTPTR_MAX - 15), fwd, QL, "address space");
    REFUSE(bootstrap, a.row_loss = P(UINTPTR_MAX - 31), fwd, QL, "address space");
    REFUSE(bootstrap, a.targets_out = P(UINTPTR_MAX - 63), fwd, QL, "address space");
    REFUSE(bootstrap, a.stats = P(UINTPTR_MAX - 15), fwd, QL, "address space");
    REFUSE(bootstrap, a.workspace = P(U + 8), fwd, QL, "workspace overlaps the quantiles");
    REFUSE(bootstrap, a.workspace = P(2 * U - 56), fwd, QL, "workspace overlaps the actions");
    REFUSE(given, a.row_loss = P(3 * U + 316), fwd, QL, "row_loss overlaps the target_quantiles");
    REFUSE(given, a.targets_out = P(3 * U - 4), fwd, QL, "targets_out overlaps the target_quantiles");
    REFUSE(bootstrap, a.row_loss = P(4 * U - 60), fwd, QL, "row_loss overlaps the reward");
    REFUSE(bootstrap, a.row_loss = P(5 * U + 12), fwd, QL, "row_loss overlaps the terminated");
    REFUSE(bootstrap, a.loss = P(6 * U + 1276), fwd, QL, "loss_out overlaps the next_quantiles");
    REFUSE(bootstrap, a.stats = P(7 * U - 4), fwd, QL, "stats_out overlaps the next_quantiles_online");
    REFUSE(bootstrap, a.loss = P(8 * U), fwd, QL, "loss_out overlaps the weights");
    REFUSE(bootstrap, a.row_loss = P(14 * U + 60), fwd, QL, "row_loss overlaps the discount");
    REFUSE(bootstrap, a.targets_out = P(14 * U - 316), fwd, QL, "targets_out overlaps the discount");
    REFUSE(bootstrap, a.workspace = P(14 * U - WS + 8), fwd, QL, "workspace overlaps the discount");
    REFUSE(bootstrap, a.stats = P(14 * U + 32), fwd, QL, "stats_out overlaps the discount");
    REFUSE(bootstrap, a.ld = 25; a.stats = P(U + 15 * 100 + 76), fwd, QL, "stats_out overlaps the quantiles"); /* the last strided row */
    REFUSE(bootstrap, a.row_loss = P(9 * U + WS - 4), fwd, QL, "outputs workspace and row_loss overlap");
    REFUSE(bootstrap, a.loss = P(9 * U + 32), fwd, QL, "outputs workspace and loss_out overlap");
    REFUSE(bootstrap, a.targets_out = P(10 * U + 60), fwd, QL, "outputs row_loss and targets_out overlap");
    REFUSE(bootstrap, a.loss = P(11 * U + 316), fwd, QL, "outputs targets_out and loss_out overlap");
    REFUSE(bootstrap, a.stats = P(10 * U - 4), fwd, QL, "outputs row_loss and stats_out overlap");
    REFUSE(bootstrap, a.stats = P(12 * U - 28), fwd, QL, "outputs loss_out and stats_out overlap");

    /* ---- the backward's own ---- */
    REFUSE(bootstrap, a.grad_loss = NULL, bwd, QB, "grad_loss pointer is NULL");
    REFUSE(bootstrap, a.grad = NULL, bwd, QB, "grad_quantiles pointer is NULL");
    REFUSE(bootstrap, a.grad_loss = P(9 * U + 2), bwd, QB, "grad_loss pointer");
    REFUSE(bootstrap, a.grad = P(10 * U + 1), bwd, QB, "grad_quantiles pointer");
    REFUSE(bootstrap, a.grad_loss = P(UINTPTR_MAX - 3), bwd, QB, "address space");
    REFUSE(bootstrap, a.grad = P(UINTPTR_MAX - 63), bwd, QB, "address space");
    REFUSE(bootstrap, a.grad = P(U + 1276), bwd, QB, "grad_quantiles overlaps the quantiles");
    REFUSE(bootstrap, a.grad = P(2 * U - 1276), bwd, QB, "grad_quantiles overlaps the actions");
    REFUSE(given, a.grad = P(3 * U + 316), bwd, QB, "grad_quantiles overlaps the target_quantiles");
    REFUSE(bootstrap, a.grad = P(6 * U - 4), bwd, QB, "grad_quantiles overlaps the next_quantiles");
    REFUSE(bootstrap, a.grad = P(8 * U + 60), bwd, QB, "grad_quantiles overlaps the weights");
    REFUSE(bootstrap, a.grad = P(14 * U - 1276), bwd, QB, "grad_quantiles overlaps the discount");
    REFUSE(bootstrap, a.grad = P(9 * U - 1276), bwd, QB, "grad_quantiles overlaps the grad_loss");

    /* ---- the expected values' own ---- */
    REFUSE(bootstrap, a.q_out = NULL, qv, QQ, "q_out pointer is NULL");
    REFUSE(bootstrap, a.q_out = P(9 * U + 2), qv, QQ, "q_out pointer");
    REFUSE(bootstrap, a.q_out = P(UINTPTR_MAX - 63), qv, QQ, "address space");
    REFUSE(bootstrap, a.q_out = P(U + 1276), qv, QQ, "q_out overlaps the quantiles");
    REFUSE(bootstrap, a.q_out = P(U - 252), qv, QQ, "q_out overlaps the quantiles");

    /* the slot is this header's own: a refusal of a call of the categorical loss header lands in its slot and leaves this one alone */
    ++calls;
    if (mxv_c51_workspace_bytes(1) != 48 + 64 ||
        mxv_c51_q_values(NULL, 0, 4, 5, (const float *)P(U), 20, -1.0, 1.0, (float *)P(9 * U)) != MXV_ERR_INVALID_ARG ||
        !strstr(mxv_c51_last_error(), "mxv_c51_q_values") || !strstr(mxv_qr_last_error(), QQ)) {
        ++bad;
        printf("BAD: the two headers' error slots are not separate: '%s' / '%s'\n", mxv_c51_last_error(), mxv_qr_last_error());
    }
    printf("qr_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
