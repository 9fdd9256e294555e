/* The argument checks of the calls of include/mxv_targets.h driven from plain C: every call below must be refused with MXV_ERR_INVALID_ARG
 * and a message that names the call — in the header's own error slot, mxv_targets_last_error — before the device is touched (the
 * addresses are invented and never dereferenced).  Built by tests/test_targets_args_sanitized.py with AddressSanitizer + UBSan against
 * the sanitized library, so the host validation — the stride and range arithmetic at the 2^40 bound and at the top of the address space,
 * the alignment and overlap loops over five inputs and two outputs, the thread-local error slot — runs instrumented. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "mxv_c51.h"
#include "mxv_targets.h"

#define P(x) ((void *)(uintptr_t)(x))
#define U 0x1000000ull
#define ROWS 16
static int calls = 0, bad = 0;

/* next U, online 2U, reward 3U, terminated 4U, discount 5U, out 6U, clipped_mass_out 7U; a row is A = 4 actions of W = 5 atoms or
 * quantiles (of one value for the scalar head) */
typedef struct {
    int64_t M;
    int32_t A, W;
    void *next;
    int64_t next_ld;
    void *online;
    int64_t online_ld;
    void *reward, *terminated;
    double gamma;
    void *discount;
    double v_min, v_max;
    void *out, *clipped;
} Args;

static Args heads(void) {
    Args a = {ROWS, 4, 5, P(U), 20, P(2 * U), 20, P(3 * U), P(4 * U), 0.99, P(5 * U), -10.0, 10.0, P(6 * U), P(7 * U)};
    return a;
}

static Args scalar(void) {
    Args a = heads();
    a.W = 1;
    a.next_ld = a.online_ld = 4;
    return a;
}

static int dqn(const Args *a) {
    return mxv_targets_dqn(NULL, a->M, a->A, (const float *)a->next, a->next_ld, (const float *)a->online, a->online_ld, (const float *)a->reward,
                           (const uint8_t *)a->terminated, a->gamma, (const float *)a->discount, (float *)a->out);
}

static int c51(const Args *a) {
    return mxv_targets_c51(NULL, a->M, a->A, a->W, (const float *)a->next, a->next_ld, (const float *)a->online, a->online_ld,
                           (const float *)a->reward, (const uint8_t *)a->terminated, a->gamma, (const float *)a->discount, a->v_min, a->v_max,
                           (float *)a->out, (float *)a->clipped);
}

static int qr(const Args *a) {
    return mxv_targets_qr(NULL, a->M, a->A, a->W, (const float *)a->next, a->next_ld, (const float *)a->online, a->online_ld, (const float *)a->reward,
                          (const uint8_t *)a->terminated, a->gamma, (const float *)a->discount, (float *)a->out);
}

static void expect(int rc, const char *api, const char *what) {
    const char *msg = mxv_targets_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what) || strncmp(msg, api, strlen(api)) != 0 || msg[strlen(api)] != ':') {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s: ... %s'\n", rc, msg ? msg : "(null)", api, what);
    }
}

#define TD "mxv_targets_dqn"
#define TC "mxv_targets_c51"
#define TQ "mxv_targets_qr"
/* one refused call: START from heads() or scalar(), EDIT the arguments, CALL dqn, c51 or qr */
#define REFUSE(START, EDIT, CALL, API, WHAT) \
    do {                                      \
        Args a = START();                     \
        EDIT;                                 \
        expect(CALL(&a), API, WHAT);          \
    } while (0)
/* what the three calls check alike */
#define ALL(EDIT, WHAT)                    \
    REFUSE(scalar, EDIT, dqn, TD, WHAT);   \
    REFUSE(heads, EDIT, c51, TC, WHAT);    \
    REFUSE(heads, EDIT, qr, TQ, WHAT)
/* ... and the two heads whose rows are A * W wide */
#define HEADS(EDIT, WHAT)                  \
    REFUSE(heads, EDIT, c51, TC, WHAT);    \
    REFUSE(heads, EDIT, qr, TQ, WHAT)

int main(void) {
    const int64_t big = (int64_t)1 << 40;
    const char *before = mxv_targets_last_error();
    ++calls;
    if (!before || before[0] != '\0') {
        ++bad;
        printf("BAD: the slot is not empty before the first call\n");
    }

    /* ---- NULL pointers, the sizes, the strides ---- */
    REFUSE(scalar, a.next = NULL, dqn, TD, "next_q pointer is NULL");
    REFUSE(heads, a.next = NULL, c51, TC, "next_logits pointer is NULL");
    REFUSE(heads, a.next = NULL, qr, TQ, "next_quantiles pointer is NULL");
    ALL(a.reward = NULL, "reward pointer is NULL");
    ALL(a.terminated = NULL, "terminated pointer is NULL");
    REFUSE(scalar, a.out = NULL, dqn, TD, "targets_out pointer is NULL");
    REFUSE(heads, a.out = NULL, c51, TC, "target_probs_out pointer is NULL");
    REFUSE(heads, a.out = NULL, qr, TQ, "target_quantiles_out pointer is NULL");
    ALL(a.M = 0, "M =");
    ALL(a.M = -3, "M =");
    ALL(a.M = INT64_MIN, "M =");
    ALL(a.M = big + 1, "2^40");
    ALL(a.M = INT64_MAX, "2^40");
    ALL(a.A = 0, "A =");
    ALL(a.A = -1, "A =");
    ALL(a.A = 65, "A =");
    REFUSE(scalar, a.next_ld = 3, dqn, TD, "next_q_ld =");
    REFUSE(scalar, a.next_ld = -4, dqn, TD, "next_q_ld =");
    REFUSE(scalar, a.online_ld = 0, dqn, TD, "next_q_online_ld =");
    REFUSE(heads, a.next_ld = 19, c51, TC, "next_logits_ld =");
    REFUSE(heads, a.A = 64; a.W = 64; a.next_ld = 4095, c51, TC, "next_logits_ld =");
    REFUSE(heads, a.online_ld = 0, c51, TC, "next_logits_online_ld =");
    REFUSE(heads, a.next_ld = 19, qr, TQ, "next_quantiles_ld =");
    REFUSE(heads, a.A = 64; a.W = 64; a.online_ld = 4095; a.next_ld = 4096, qr, TQ, "next_quantiles_online_ld =");
    ALL(a.next_ld = INT64_MAX, "beyond 2^40 elements");
    ALL(a.online_ld = INT64_MAX, "beyond 2^40 elements");
    ALL(a.M = big; a.next_ld = 21, "beyond 2^40 elements");

    /* ---- the heads' own: the atoms and the support, the quantiles ---- */
    REFUSE(heads, a.W = 1, c51, TC, "Z =");
    REFUSE(heads, a.W = 0, c51, TC, "Z =");
    REFUSE(heads, a.W = -7, c51, TC, "Z =");
    REFUSE(heads, a.W = 65, c51, TC, "Z =");
    REFUSE(heads, a.v_min = NAN, c51, TC, "must be finite");
    REFUSE(heads, a.v_max = INFINITY, c51, TC, "must be finite");
    REFUSE(heads, a.v_min = -INFINITY, c51, TC, "must be finite");
    REFUSE(heads, a.v_min = 10.0, c51, TC, "must be below v_max");
    REFUSE(heads, a.v_min = 11.0, c51, TC, "must be below v_max");
    REFUSE(heads, a.W = 0, qr, TQ, "N =");
    REFUSE(heads, a.W = -7, qr, TQ, "N =");
    REFUSE(heads, a.W = 65, qr, TQ, "N =");

    /* ---- the scalar: gamma is checked beside a discount too ---- */
    ALL(a.gamma = INFINITY, "gamma =");
    ALL(a.gamma = -INFINITY, "gamma =");
    ALL(a.gamma = NAN, "gamma =");
    ALL(a.discount = NULL; a.gamma = NAN, "gamma =");

    /* ---- alignment and the top of the address space ---- */
    ALL(a.next = P(U + 2), "pointer");
    ALL(a.online = P(2 * U + 1), "_online pointer");
    ALL(a.reward = P(3 * U + 3), "reward pointer");
    ALL(a.discount = P(5 * U + 2), "discount pointer");
    ALL(a.out = P(6 * U + 2), "_out pointer");
    REFUSE(heads, a.clipped = P(7 * U + 1), c51, TC, "clipped_mass_out pointer");
    ALL(a.next = P(UINTPTR_MAX - 15), "address space");
    ALL(a.online = P(UINTPTR_MAX - 15), "address space");
    ALL(a.reward = P(UINTPTR_MAX - 15), "address space");
    ALL(a.terminated = P(UINTPTR_MAX - 3), "address space");
    ALL(a.discount = P(UINTPTR_MAX - 31), "address space");
    ALL(a.out = P(UINTPTR_MAX - 15), "address space");
    REFUSE(heads, a.clipped = P(UINTPTR_MAX - 31), c51, TC, "address space");

    /* ---- an output shares a byte with an input or with the other output ---- */
    REFUSE(scalar, a.out = P(U + 252), dqn, TD, "targets_out overlaps the next_q");
    REFUSE(scalar, a.next_ld = 9; a.out = P(U + 15 * 36 + 12), dqn, TD, "targets_out overlaps the next_q"); /* the last strided row */
    REFUSE(scalar, a.out = P(2 * U - 60), dqn, TD, "targets_out overlaps the next_q_online");
    REFUSE(heads, a.out = P(U + 1276), c51, TC, "target_probs_out overlaps the next_logits");
    REFUSE(heads, a.out = P(2 * U - 316), c51, TC, "target_probs_out overlaps the next_logits_online");
    REFUSE(heads, a.out = P(U + 1276), qr, TQ, "target_quantiles_out overlaps the next_quantiles");
    REFUSE(heads, a.out = P(2 * U - 316), qr, TQ, "target_quantiles_out overlaps the next_quantiles_online");
    ALL(a.out = P(3 * U + 60), "_out overlaps the reward");
    ALL(a.out = P(4 * U + 12), "_out overlaps the terminated");
    ALL(a.out = P(5 * U + 60), "_out overlaps the discount");
    REFUSE(heads, a.clipped = P(U + 1276), c51, TC, "clipped_mass_out overlaps the next_logits");
    REFUSE(heads, a.clipped = P(3 * U - 60), c51, TC, "clipped_mass_out overlaps the reward");
    REFUSE(heads, a.clipped = P(4 * U + 12), c51, TC, "clipped_mass_out overlaps the terminated");
    REFUSE(heads, a.clipped = P(5 * U + 60), c51, TC, "clipped_mass_out overlaps the discount");
    REFUSE(heads, a.clipped = P(6 * U + 316), c51, TC, "outputs target_probs_out and clipped_mass_out overlap");
    REFUSE(heads, a.clipped = P(6 * U - 60), c51, TC, "outputs target_probs_out and clipped_mass_out overlap");

    /* the slot is this header's own: a refusal of a categorical-loss call lands in mxv_c51_last_error and leaves this one alone */
    ++calls;
    if (mxv_c51_q_values(NULL, 0, 4, 5, (const float *)P(U), 20, -10.0, 10.0, (float *)P(9 * U)) != MXV_ERR_INVALID_ARG ||
        !strstr(mxv_c51_last_error(), "mxv_c51_q_values") || !strstr(mxv_targets_last_error(), TC) || strstr(mxv_targets_last_error(), "mxv_c51_q_values")) {
        ++bad;
        printf("BAD: the two headers' error slots are not separate: '%s' / '%s'\n", mxv_c51_last_error(), mxv_targets_last_error());
    }
    printf("targets_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
