/* The argument checks of the calls of include/mxv_replay.h driven from plain C: every call below must be refused with
 * MXV_ERR_INVALID_ARG and a message that names the call — in the header's own error slot, mxv_replay_last_error — before the device is
 * touched (the addresses are invented and never dereferenced).  Built by tests/test_replay_args_sanitized.py with AddressSanitizer +
 * UBSan against the sanitized library, so the host validation — the K * N and C * W arithmetic at the 2^31 and 2^40 bounds, the stride
 * and range arithmetic at the top of the address space, the alignment and overlap loops over eight inputs and five or six outputs, the
 * thread-local error slot — runs instrumented. */
#include <stdio.h>
#include <string.h>

#include "mxv_dqn.h"
#include "mxv_replay.h"

#define P(x) ((void *)(uintptr_t)(x))
#define U 0x1000000ull
static int calls = 0, bad = 0;

/* insert: first_obs U, obs 2U, final_obs 3U, actions 4U, reward 5U, terminated 6U, truncated 7U, state_dev 8U, the ring 9U .. 13U;
 * sample: indices 14U, obs_out 15U, next_out 16U, action_out 17U, reward_out 18U, term_out 19U */
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
    uint64_t seed, count, step;
    void *state_dev, *ring_obs, *ring_next, *ring_action, *ring_reward, *ring_term;
    void *indices, *obs_out, *next_out, *action_out, *reward_out, *term_out;
} Args;

static Args base(void) {
    Args a = {64, 4, 2, 8, 16, P(U), 4, P(2 * U), 4, P(3 * U), 4, P(4 * U), 8, P(5 * U), 8, P(6 * U), P(7 * U), 1, 5, 0,
              P(8 * U), P(9 * U), P(10 * U), P(11 * U), P(12 * U), P(13 * U), P(14 * U), P(15 * U), P(16 * U), P(17 * U), P(18 * U), P(19 * U)};
    return a;
}

static int ins(const Args *a) {
    return mxv_replay_insert(NULL, a->C, a->W, a->K, a->N, a->first_obs, a->first_ld, a->obs, a->obs_ld, a->final_obs, a->final_ld, a->actions,
                             a->action_bytes, a->reward, a->reward_bytes, (const uint8_t *)a->terminated, (const uint8_t *)a->truncated, a->count,
                             (uint64_t *)a->state_dev, a->ring_obs, a->ring_next, a->ring_action, (float *)a->ring_reward, (uint8_t *)a->ring_term);
}

static int smp(const Args *a) {
    return mxv_replay_sample(NULL, a->C, a->W, a->B, a->ring_obs, a->ring_next, a->ring_action, (const float *)a->ring_reward,
                             (const uint8_t *)a->ring_term, a->seed, a->count, a->step, (uint64_t *)a->state_dev, (int64_t *)a->indices, a->obs_out,
                             a->next_out, a->action_out, a->action_bytes, (float *)a->reward_out, (uint8_t *)a->term_out);
}

static void expect(int rc, const char *api, const char *what) {
    const char *msg = mxv_replay_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what) || strncmp(msg, api, strlen(api)) != 0 || msg[strlen(api)] != ':') {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s: ... %s'\n", rc, msg ? msg : "(null)", api, what);
    }
}

#define RI "mxv_replay_insert"
#define RS "mxv_replay_sample"
#define REFUSE(EDIT, CALL, API, WHAT) \
    do {                               \
        Args a = base();               \
        EDIT;                          \
        expect(CALL(&a), API, WHAT);   \
    } while (0)
#define INS(EDIT, WHAT) REFUSE(EDIT, ins, RI, WHAT)
#define SMP(EDIT, WHAT) REFUSE(EDIT, smp, RS, WHAT)
/* what both entry points check alike */
#define BOTH(EDIT, WHAT) \
    INS(EDIT, WHAT);     \
    SMP(EDIT, WHAT)

int main(void) {
    const int64_t cap = (int64_t)1 << 31;
    const char *before = mxv_replay_last_error();
    ++calls;
    if (!before || before[0] != '\0') {
        ++bad;
        printf("BAD: the slot is not empty before the first call\n");
    }

    /* ---- the ring ---- */
    BOTH(a.C = 0, "C =");
    BOTH(a.C = -1, "C =");
    BOTH(a.C = INT64_MIN, "C =");
    BOTH(a.C = cap + 1, "C =");
    BOTH(a.C = INT64_MAX, "C =");
    BOTH(a.W = 0, "W =");
    BOTH(a.W = -3, "W =");
    BOTH(a.W = 65537, "W =");
    BOTH(a.W = INT32_MAX, "W =");
    BOTH(a.C = cap; a.W = 1024, "C * W =");
    BOTH(a.C = cap; a.W = 65536, "C * W =");
    BOTH(a.action_bytes = 0, "action_bytes =");
    BOTH(a.action_bytes = 2, "action_bytes =");
    BOTH(a.action_bytes = 16, "action_bytes =");
    BOTH(a.count = ((uint64_t)1 << 63) + 1, "count =");
    BOTH(a.count = UINT64_MAX, "count =");
    BOTH(a.ring_obs = NULL, "ring_obs pointer is NULL");
    BOTH(a.ring_next = NULL, "ring_next pointer is NULL");
    BOTH(a.ring_action = NULL, "ring_action pointer is NULL");
    BOTH(a.ring_reward = NULL, "ring_reward pointer is NULL");
    BOTH(a.ring_term = NULL, "ring_term pointer is NULL");
    BOTH(a.state_dev = P(8 * U + 4), "state_dev pointer");
    BOTH(a.ring_obs = P(9 * U + 2), "ring_obs pointer");
    BOTH(a.ring_next = P(10 * U + 1), "ring_next pointer");
    BOTH(a.ring_action = P(11 * U + 2), "ring_action pointer");
    BOTH(a.ring_reward = P(12 * U + 3), "ring_reward pointer");
    BOTH(a.ring_obs = P(UINTPTR_MAX - 15), "address space");
    BOTH(a.ring_action = P(UINTPTR_MAX - 15), "address space");
    BOTH(a.ring_term = P(UINTPTR_MAX - 7), "address space");
    BOTH(a.state_dev = P(UINTPTR_MAX - 7), "address space");

    /* ---- insert: pointers, sizes, strides, widths ---- */
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

    /* ---- insert: the five ring arrays against the inputs, state_dev and each other ---- */
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
    INS(a.ring_next = P(9 * U + 1020), "outputs ring_obs and ring_next overlap");
    INS(a.ring_action = P(9 * U - 252), "outputs ring_obs and ring_action overlap");
    INS(a.ring_reward = P(9 * U + 512), "outputs ring_obs and ring_reward overlap");
    INS(a.ring_term = P(10 * U), "outputs ring_next and ring_term overlap");
    INS(a.ring_reward = P(11 * U + 252), "outputs ring_action and ring_reward overlap");
    INS(a.ring_term = P(12 * U + 255), "outputs ring_reward and ring_term overlap");

    /* ---- sample ---- */
    SMP(a.indices = NULL, "indices pointer is NULL");
    SMP(a.obs_out = NULL, "obs_out pointer is NULL");
    SMP(a.next_out = NULL, "next_out pointer is NULL");
    SMP(a.action_out = NULL, "action_out pointer is NULL");
    SMP(a.reward_out = NULL, "reward_out pointer is NULL");
    SMP(a.term_out = NULL, "term_out pointer is NULL");
    SMP(a.B = 0, "B =");
    SMP(a.B = -7, "B =");
    SMP(a.B = INT64_MIN, "B =");
    SMP(a.B = ((int64_t)1 << 38) + 1, "B * W =");
    SMP(a.B = INT64_MAX, "B * W =");
    SMP(a.indices = P(14 * U + 4), "indices pointer");
    SMP(a.obs_out = P(15 * U + 2), "obs_out pointer");
    SMP(a.next_out = P(16 * U + 1), "next_out pointer");
    SMP(a.action_out = P(17 * U + 4), "action_out pointer");
    SMP(a.action_bytes = 4; a.action_out = P(17 * U + 2), "action_out pointer");
    SMP(a.reward_out = P(18 * U + 2), "reward_out pointer");
    SMP(a.indices = P(UINTPTR_MAX - 15), "address space");
    SMP(a.obs_out = P(UINTPTR_MAX - 15), "address space");
    SMP(a.term_out = P(UINTPTR_MAX - 7), "address space");
    SMP(a.indices = P(9 * U + 1016), "indices overlaps the ring_obs");
    SMP(a.obs_out = P(10 * U - 252), "obs_out overlaps the ring_next");
    SMP(a.next_out = P(11 * U + 252), "next_out overlaps the ring_action");
    SMP(a.action_out = P(12 * U - 120), "action_out overlaps the ring_reward");
    SMP(a.reward_out = P(13 * U + 60), "reward_out overlaps the ring_term");
    SMP(a.term_out = P(8 * U + 15), "term_out overlaps state_dev");
    SMP(a.reward_out = P(8 * U - 60), "reward_out overlaps state_dev");
    SMP(a.obs_out = P(14 * U + 120), "outputs indices and obs_out overlap");
    SMP(a.next_out = P(15 * U + 252), "outputs obs_out and next_out overlap");
    SMP(a.action_out = P(16 * U - 120), "outputs next_out and action_out overlap");
    SMP(a.reward_out = P(17 * U + 124), "outputs action_out and reward_out overlap");
    SMP(a.term_out = P(18 * U + 63), "outputs reward_out and term_out overlap");
    SMP(a.term_out = P(14 * U), "outputs indices and term_out overlap");

    /* count = 2^63 itself is accepted: the call gets as far as the next check */
    INS(a.count = (uint64_t)1 << 63; a.ring_term = P(10 * U), "outputs ring_next and ring_term overlap");
    SMP(a.count = (uint64_t)1 << 63; a.term_out = P(14 * U), "outputs indices and term_out overlap");

    /* the slot is this header's own: a refusal of a Q-learning loss call lands in mxv_dqn_last_error and leaves this one alone */
    ++calls;
    if (mxv_dqn_workspace_bytes(0) != 0 ||
        mxv_dqn_loss(NULL, 0, 4, (const float *)P(U), 4, P(2 * U), 8, NULL, NULL, NULL, NULL, 0, NULL, 0, 0.99, 1.0, NULL, NULL, 0, NULL, NULL, NULL) !=
            MXV_ERR_INVALID_ARG ||
        !strstr(mxv_dqn_last_error(), "mxv_dqn_loss") || !strstr(mxv_replay_last_error(), RS)) {
        ++bad;
        printf("BAD: the two headers' error slots are not separate: '%s' / '%s'\n", mxv_dqn_last_error(), mxv_replay_last_error());
    }
    printf("replay_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
