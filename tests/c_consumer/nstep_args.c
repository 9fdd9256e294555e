/* The argument checks of the calls of include/mxv_nstep.h driven from plain C: every call below must be refused with
 * MXV_ERR_INVALID_ARG and a message that names the call — in the header's own error slot, mxv_nstep_last_error — before the device is
 * touched (the addresses are invented and never dereferenced).  Built by tests/test_nstep_args_sanitized.py with AddressSanitizer +
 * UBSan against the sanitized library, so the host validation — the window and discount bounds, the K * N and C * W arithmetic at the
 * 2^31 and 2^40 bounds, the stride and range arithmetic at the top of the address space, the alignment and overlap loops over eight
 * inputs and six outputs, the thread-local error slot — runs instrumented. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "mxv_nstep.h"
#include "mxv_replay.h"

#define P(x) ((void *)(uintptr_t)(x))
#define U 0x1000000ull
static int calls = 0, bad = 0;

/* insert: first_obs U, obs 2U, final_obs 3U, actions 4U, reward 5U, terminated 6U, truncated 7U, state_dev 8U, the ring 9U .. 13U,
 * ring_discount 14U; gather: indices 15U, discount_out 16U */
typedef struct {
    int64_t C;
    int32_t W;
    int64_t K, N, B;
    void *first_obs;
    int64_t first_ld;
    void *obs;
    int64_t obs_ld;
    void *final_obs;
    int64_t final_ld;
    void *actions;
    int32_t action_bytes;
    void *reward;
    int32_t reward_bytes;
    void *terminated, *truncated;
    uint64_t count;
    void *state_dev, *ring_obs, *ring_next, *ring_action, *ring_reward, *ring_term;
    int32_t n;
    double gamma;
    void *ring_discount, *indices, *discount_out;
} Args;

static Args base(void) {
    Args a = {64,       4,        2,         8,         16,        P(U),      4,         P(2 * U),  4,    P(3 * U), 4,         P(4 * U),  8,         P(5 * U),
              8,        P(6 * U), P(7 * U),  5,         P(8 * U),  P(9 * U),  P(10 * U), P(11 * U), P(12 * U), P(13 * U), 3,   0.99,     P(14 * U), P(15 * U),
              P(16 * U)};
    return a;
}

static int ins(const Args *a) {
    return mxv_nstep_insert(NULL, a->C, a->W, a->K, a->N, a->first_obs, a->first_ld, a->obs, a->obs_ld, a->final_obs, a->final_ld, a->actions,
                            a->action_bytes, a->reward, a->reward_bytes, (const uint8_t *)a->terminated, (const uint8_t *)a->truncated, a->count,
                            (uint64_t *)a->state_dev, a->ring_obs, a->ring_next, a->ring_action, (float *)a->ring_reward, (uint8_t *)a->ring_term, a->n,
                            a->gamma, (float *)a->ring_discount);
}

static int gat(const Args *a) {
    return mxv_nstep_gather(NULL, a->C, a->B, (const float *)a->ring_discount, (const int64_t *)a->indices, (float *)a->discount_out);
}

static void expect(int rc, const char *api, const char *what) {
    const char *msg = mxv_nstep_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what) || strncmp(msg, api, strlen(api)) != 0 || msg[strlen(api)] != ':') {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s: ... %s'\n", rc, msg ? msg : "(null)", api, what);
    }
}

#define NI "mxv_nstep_insert"
#define NG "mxv_nstep_gather"
#define REFUSE(EDIT, CALL, API, WHAT) \
    do {                               \
        Args a = base();               \
        EDIT;                          \
        expect(CALL(&a), API, WHAT);   \
    } while (0)
#define INS(EDIT, WHAT) REFUSE(EDIT, ins, NI, WHAT)
#define GAT(EDIT, WHAT) REFUSE(EDIT, gat, NG, WHAT)
/* what both entry points check alike */
#define BOTH(EDIT, WHAT) \
    INS(EDIT, WHAT);     \
    GAT(EDIT, WHAT)

int main(void) {
    const int64_t cap = (int64_t)1 << 31;
    const char *before = mxv_nstep_last_error();
    ++calls;
    if (!before || before[0] != '\0') {
        ++bad;
        printf("BAD: the slot is not empty before the first call\n");
    }

    /* ---- both ---- */
    BOTH(a.C = 0, "C =");
    BOTH(a.C = -1, "C =");
    BOTH(a.C = INT64_MIN, "C =");
    BOTH(a.C = cap + 1, "C =");
    BOTH(a.C = INT64_MAX, "C =");
    BOTH(a.ring_discount = NULL, "ring_discount pointer is NULL");
    BOTH(a.ring_discount = P(14 * U + 2), "ring_discount pointer");
    BOTH(a.ring_discount = P(UINTPTR_MAX - 15), "address space");

    /* ---- the window ---- */
    INS(a.n = 0, "n =");
    INS(a.n = -1, "n =");
    INS(a.n = 65, "n =");
    INS(a.n = INT32_MAX, "n =");
    INS(a.n = INT32_MIN, "n =");
    INS(a.gamma = NAN, "gamma =");
    INS(a.gamma = -NAN, "gamma =");
    INS(a.gamma = -1e-300, "gamma =");
    INS(a.gamma = -1.0, "gamma =");
    INS(a.gamma = 1.0000000000000002, "gamma =");
    INS(a.gamma = INFINITY, "gamma =");
    INS(a.gamma = -INFINITY, "gamma =");
    INS(a.gamma = 1e308, "gamma =");

    /* ---- insert: the ring, pointers, sizes, strides, widths ---- */
    INS(a.W = 0, "W =");
    INS(a.W = -3, "W =");
    INS(a.W = 65537, "W =");
    INS(a.W = INT32_MAX, "W =");
    INS(a.C = cap; a.W = 1024, "C * W =");
    INS(a.C = cap; a.W = 65536, "C * W =");
    INS(a.action_bytes = 0, "action_bytes =");
    INS(a.action_bytes = 2, "action_bytes =");
    INS(a.action_bytes = 16, "action_bytes =");
    INS(a.count = ((uint64_t)1 << 63) + 1, "count =");
    INS(a.count = UINT64_MAX, "count =");
    INS(a.ring_obs = NULL, "ring_obs pointer is NULL");
    INS(a.ring_next = NULL, "ring_next pointer is NULL");
    INS(a.ring_action = NULL, "ring_action pointer is NULL");
    INS(a.ring_reward = NULL, "ring_reward pointer is NULL");
    INS(a.ring_term = NULL, "ring_term pointer is NULL");
    INS(a.state_dev = P(8 * U + 4), "state_dev pointer");
    INS(a.ring_obs = P(9 * U + 2), "ring_obs pointer");
    INS(a.ring_next = P(10 * U + 1), "ring_next pointer");
    INS(a.ring_action = P(11 * U + 2), "ring_action pointer");
    INS(a.ring_reward = P(12 * U + 3), "ring_reward pointer");
    INS(a.ring_obs = P(UINTPTR_MAX - 15), "address space");
    INS(a.ring_action = P(UINTPTR_MAX - 15), "address space");
    INS(a.ring_term = P(UINTPTR_MAX - 7), "address space");
    INS(a.state_dev = P(UINTPTR_MAX - 7), "address space");
    INS(a.first_obs = NULL, "first_obs pointer is NULL");
    INS(a.obs = NULL, "obs pointer is NULL");
    INS(a.actions = NULL, "actions pointer is NULL");
    INS(a.reward = NULL, "reward pointer is NULL");
    INS(a.terminated = NULL, "terminated pointer is NULL");
    INS(a.K = 0, "K =");
    INS(a.K = -2, "K =");
    INS(a.K = INT64_MIN, "K =");
    INS(a.N = 0, "N =");
    INS(a.N = INT64_MIN, "N =");
    INS(a.K = 9, "exceed C");
    INS(a.C = 15, "exceed C");
    INS(a.K = INT64_MAX; a.N = INT64_MAX, "exceed C");
    INS(a.K = (int64_t)1 << 32; a.N = (int64_t)1 << 32, "exceed C"); /* the product wraps to 0 */
    INS(a.first_ld = 3, "first_obs_ld =");
    INS(a.first_ld = INT64_MIN, "first_obs_ld =");
    INS(a.obs_ld = 3, "obs_ld =");
    INS(a.final_ld = -4, "final_obs_ld =");
    INS(a.obs_ld = (int64_t)1 << 40, "beyond 2^40 elements");
    INS(a.first_ld = INT64_MAX, "beyond 2^40 elements");
    INS(a.final_ld = (int64_t)1 << 38, "beyond 2^40 elements");
    INS(a.reward_bytes = 0, "reward_bytes =");
    INS(a.reward_bytes = 2, "reward_bytes =");
    INS(a.reward_bytes = 16, "reward_bytes =");
    INS(a.final_obs = NULL, "truncated is given without final_obs");
    INS(a.first_obs = P(U + 2), "first_obs pointer");
    INS(a.obs = P(2 * U + 1), "obs pointer");
    INS(a.final_obs = P(3 * U + 3), "final_obs pointer");
    INS(a.actions = P(4 * U + 4), "actions pointer");
    INS(a.action_bytes = 4; a.actions = P(4 * U + 2), "actions pointer");
    INS(a.reward = P(5 * U + 4), "reward pointer");
    INS(a.reward_bytes = 4; a.reward = P(5 * U + 2), "reward pointer");
    INS(a.first_obs = P(UINTPTR_MAX - 15), "address space");
    INS(a.obs = P(UINTPTR_MAX - 15), "address space");
    INS(a.final_obs = P(UINTPTR_MAX - 63), "address space");
    INS(a.actions = P(UINTPTR_MAX - 7), "address space");
    INS(a.terminated = P(UINTPTR_MAX - 7), "address space");
    INS(a.truncated = P(UINTPTR_MAX - 3), "address space");

    /* ---- insert: the six ring arrays against the inputs, state_dev and each other ---- */
    INS(a.ring_obs = P(U + 16), "ring_obs overlaps the first_obs");
    INS(a.ring_next = P(2 * U - 1020), "ring_next overlaps the obs");
    INS(a.ring_action = P(3 * U + 252), "ring_action overlaps the final_obs");
    INS(a.ring_reward = P(4 * U + 124), "ring_reward overlaps the actions");
    INS(a.ring_reward = P(5 * U - 252), "ring_reward overlaps the reward");
    INS(a.ring_term = P(6 * U + 15), "ring_term overlaps the terminated");
    INS(a.ring_term = P(7 * U - 63), "ring_term overlaps the truncated");
    INS(a.ring_obs = P(8 * U - 1008), "ring_obs overlaps state_dev");
    INS(a.ring_term = P(8 * U + 15), "ring_term overlaps state_dev");
    INS(a.obs_ld = 7; a.ring_action = P(2 * U + 15 * 28 + 12), "ring_action overlaps the obs"); /* the last strided row */
    INS(a.ring_discount = P(U + 60), "ring_discount overlaps the first_obs");
    INS(a.ring_discount = P(3 * U - 252), "ring_discount overlaps the final_obs");
    INS(a.ring_discount = P(5 * U + 124), "ring_discount overlaps the reward");
    INS(a.ring_discount = P(6 * U - 252), "ring_discount overlaps the terminated");
    INS(a.ring_discount = P(7 * U + 12), "ring_discount overlaps the truncated");
    INS(a.ring_discount = P(8 * U + 12), "ring_discount overlaps state_dev");
    INS(a.ring_next = P(9 * U + 1020), "outputs ring_obs and ring_next overlap");
    INS(a.ring_action = P(9 * U - 252), "outputs ring_obs and ring_action overlap");
    INS(a.ring_reward = P(9 * U + 512), "outputs ring_obs and ring_reward overlap");
    INS(a.ring_term = P(10 * U), "outputs ring_next and ring_term overlap");
    INS(a.ring_reward = P(11 * U + 252), "outputs ring_action and ring_reward overlap");
    INS(a.ring_term = P(12 * U + 255), "outputs ring_reward and ring_term overlap");
    INS(a.ring_discount = P(9 * U + 1020), "outputs ring_obs and ring_discount overlap");
    INS(a.ring_discount = P(10 * U - 252), "outputs ring_next and ring_discount overlap");
    INS(a.ring_discount = P(11 * U + 252), "outputs ring_action and ring_discount overlap");
    INS(a.ring_discount = P(12 * U - 252), "outputs ring_reward and ring_discount overlap");
    INS(a.ring_discount = P(13 * U + 60), "outputs ring_term and ring_discount overlap");

    /* ---- gather ---- */
    GAT(a.indices = NULL, "indices pointer is NULL");
    GAT(a.discount_out = NULL, "discount_out pointer is NULL");
    GAT(a.B = 0, "B =");
    GAT(a.B = -7, "B =");
    GAT(a.B = INT64_MIN, "B =");
    GAT(a.B = ((int64_t)1 << 40) + 1, "beyond 2^40 elements");
    GAT(a.B = INT64_MAX, "beyond 2^40 elements");
    GAT(a.indices = P(15 * U + 4), "indices pointer");
    GAT(a.discount_out = P(16 * U + 1), "discount_out pointer");
    GAT(a.indices = P(UINTPTR_MAX - 15), "address space");
    GAT(a.discount_out = P(UINTPTR_MAX - 15), "address space");
    GAT(a.discount_out = P(14 * U + 252), "discount_out overlaps the ring_discount");
    GAT(a.discount_out = P(15 * U - 60), "discount_out overlaps the indices");
    GAT(a.discount_out = P(15 * U + 124), "discount_out overlaps the indices");

    /* the bounds themselves are accepted: the call gets as far as the next check */
    INS(a.n = 1; a.ring_term = P(10 * U), "outputs ring_next and ring_term overlap");
    INS(a.n = 64; a.ring_term = P(10 * U), "outputs ring_next and ring_term overlap");
    INS(a.gamma = 0.0; a.ring_term = P(10 * U), "outputs ring_next and ring_term overlap");
    INS(a.gamma = 1.0; a.ring_term = P(10 * U), "outputs ring_next and ring_term overlap");
    INS(a.count = (uint64_t)1 << 63; a.ring_term = P(10 * U), "outputs ring_next and ring_term overlap");

    /* the slot is this header's own: a refusal of the one-step insert lands in mxv_replay_last_error and leaves this one alone */
    ++calls;
    {
        Args a = base();
        if (mxv_replay_insert(NULL, 0, a.W, a.K, a.N, a.first_obs, a.first_ld, a.obs, a.obs_ld, a.final_obs, a.final_ld, a.actions, a.action_bytes, a.reward,
                              a.reward_bytes, (const uint8_t *)a.terminated, (const uint8_t *)a.truncated, a.count, (uint64_t *)a.state_dev, a.ring_obs,
                              a.ring_next, a.ring_action, (float *)a.ring_reward, (uint8_t *)a.ring_term) != MXV_ERR_INVALID_ARG ||
            !strstr(mxv_replay_last_error(), "mxv_replay_insert") || !strstr(mxv_nstep_last_error(), NI)) {
            ++bad;
            printf("BAD: the two headers' error slots are not separate: '%s' / '%s'\n", mxv_replay_last_error(), mxv_nstep_last_error());
        }
    }
    printf("nstep_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
