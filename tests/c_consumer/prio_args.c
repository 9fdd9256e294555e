/* The argument checks of the calls of include/mxv_prio.h driven from plain C: every call below must be refused with
 * MXV_ERR_INVALID_ARG and a message that names the call — in the header's own error slot, mxv_prio_last_error — before the device is
 * touched (the addresses are invented and never dereferenced).  Built by tests/test_prio_args_sanitized.py with AddressSanitizer +
 * UBSan against the sanitized library, so the host validation — the layout arithmetic at C = 2^31, the K * N, C * W and B * W
 * arithmetic at their bounds, the ranges of alpha, beta and eps with NaN, the range arithmetic at the top of the address space, the
 * alignment and overlap loops over eight inputs and eight outputs, the thread-local error slot — runs instrumented. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "mxv_prio.h"
#include "mxv_replay.h"

#define P(x) ((void *)(uintptr_t)(x))
#define U 0x1000000ull
static int calls = 0, bad = 0;

/* indices U, td_error 2U, state_dev 3U, leaf 4U, node 5U, qmax 6U, the ring 7U .. 11U, workspace 12U;
 * sample: indices 13U, obs_out 14U, next_out 15U, action_out 16U, reward_out 17U, term_out 18U, weights_out 19U, step_dev 20U */
typedef struct {
    int64_t C;
    int32_t W;
    int64_t K, N, B;
    void *indices, *td, *state_dev, *leaf;
    int64_t leaf_words;
    void *node;
    int64_t node_words;
    void *qmax;
    double alpha, eps, beta;
    uint64_t seed, count, step;
    void *ring_obs, *ring_next, *ring_action, *ring_reward, *ring_term, *workspace;
    void *indices_out, *obs_out, *next_out, *action_out;
    int32_t action_bytes;
    void *reward_out, *term_out, *weights_out, *step_dev;
} Args;

static Args base(void) {
    Args a = {64, 4, 2, 8, 16, P(U), P(2 * U), P(3 * U), P(4 * U), 64, P(5 * U), 32, P(6 * U), 0.6, 1e-6, 0.4, 1, 5, 0,
              P(7 * U), P(8 * U), P(9 * U), P(10 * U), P(11 * U), P(12 * U), P(13 * U), P(14 * U), P(15 * U), P(16 * U), 8,
              P(17 * U), P(18 * U), P(19 * U), P(20 * U)};
    return a;
}

static int ins(const Args *a) {
    return mxv_prio_insert(NULL, a->C, a->K, a->N, a->count, (const uint64_t *)a->state_dev, (uint32_t *)a->leaf, a->leaf_words,
                           (uint64_t *)a->node, a->node_words, (const uint32_t *)a->qmax);
}

static int upd(const Args *a) {
    return mxv_prio_update(NULL, a->C, a->B, (const int64_t *)a->indices, (const float *)a->td, a->alpha, a->eps, a->count,
                           (const uint64_t *)a->state_dev, (uint32_t *)a->leaf, a->leaf_words, (uint64_t *)a->node, a->node_words,
                           (uint32_t *)a->qmax, (uint32_t *)a->workspace);
}

static int smp(const Args *a) {
    return mxv_prio_sample(NULL, a->C, a->W, a->B, a->ring_obs, a->ring_next, a->ring_action, (const float *)a->ring_reward,
                           (const uint8_t *)a->ring_term, (const uint32_t *)a->leaf, a->leaf_words, (const uint64_t *)a->node, a->node_words,
                           a->seed, a->step, (uint64_t *)a->step_dev, a->beta, (uint32_t *)a->workspace, (int64_t *)a->indices_out, a->obs_out,
                           a->next_out, a->action_out, a->action_bytes, (float *)a->reward_out, (uint8_t *)a->term_out, (float *)a->weights_out);
}

static void expect(int rc, const char *api, const char *what) {
    const char *msg = mxv_prio_last_error();
    ++calls;
    if (rc != MXV_ERR_INVALID_ARG || !msg || !strstr(msg, what) || strncmp(msg, api, strlen(api)) != 0 || msg[strlen(api)] != ':') {
        ++bad;
        printf("BAD: rc=%d msg='%s' wanted '%s: ... %s'\n", rc, msg ? msg : "(null)", api, what);
    }
}

#define PI "mxv_prio_insert"
#define PU "mxv_prio_update"
#define PS "mxv_prio_sample"
#define REFUSE(EDIT, CALL, API, WHAT) \
    do {                               \
        Args a = base();               \
        EDIT;                          \
        expect(CALL(&a), API, WHAT);   \
    } while (0)
#define INS(EDIT, WHAT) REFUSE(EDIT, ins, PI, WHAT)
#define UPD(EDIT, WHAT) REFUSE(EDIT, upd, PU, WHAT)
#define SMP(EDIT, WHAT) REFUSE(EDIT, smp, PS, WHAT)
/* what all three entry points check alike: the tree */
#define ALL(EDIT, WHAT) \
    INS(EDIT, WHAT);    \
    UPD(EDIT, WHAT);    \
    SMP(EDIT, WHAT)

int main(void) {
    const int64_t cap = (int64_t)1 << 31;
    int64_t leaf_words = -1, node_words = -1;
    int32_t levels = -1;
    const char *before = mxv_prio_last_error();
    ++calls;
    if (!before || before[0] != '\0') {
        ++bad;
        printf("BAD: the slot is not empty before the first call\n");
    }

    /* ---- the layout ---- */
    ++calls;
    if (mxv_prio_layout(64, &leaf_words, &node_words, &levels) != MXV_OK || leaf_words != 64 || node_words != 32 || levels != 2 ||
        mxv_prio_layout(1, &leaf_words, &node_words, &levels) != MXV_OK || leaf_words != 16 || node_words != 16 || levels != 1 ||
        mxv_prio_layout(17, &leaf_words, NULL, NULL) != MXV_OK || leaf_words != 32 || mxv_prio_layout(cap, &leaf_words, &node_words, &levels) != MXV_OK ||
        leaf_words != cap || levels != 8 || node_words != (cap >> 4) + (cap >> 8) + (cap >> 12) + (cap >> 16) + (cap >> 20) + (cap >> 24) + 16 + 16 ||
        mxv_prio_layout(1 << 20, NULL, &node_words, &levels) != MXV_OK || levels != 5 || node_words != 65536 + 4096 + 256 + 16 + 16) {
        ++bad;
        printf("BAD: mxv_prio_layout: %lld %lld %d\n", (long long)leaf_words, (long long)node_words, (int)levels);
    }
    expect(mxv_prio_layout(0, &leaf_words, &node_words, &levels), "mxv_prio_layout", "C =");
    expect(mxv_prio_layout(cap + 1, NULL, NULL, NULL), "mxv_prio_layout", "C =");
    expect(mxv_prio_layout(INT64_MIN, NULL, NULL, NULL), "mxv_prio_layout", "C =");

    /* ---- the tree ---- */
    ALL(a.C = 0, "C =");
    ALL(a.C = -1, "C =");
    ALL(a.C = INT64_MIN, "C =");
    ALL(a.C = cap + 1, "C =");
    ALL(a.C = INT64_MAX, "C =");
    ALL(a.leaf = NULL, "leaf pointer is NULL");
    ALL(a.node = NULL, "node pointer is NULL");
    ALL(a.leaf_words = 63, "leaf_words =");
    ALL(a.leaf_words = 80, "leaf_words =");
    ALL(a.leaf_words = INT64_MIN, "leaf_words =");
    ALL(a.node_words = 16, "node_words =");
    ALL(a.node_words = 33, "node_words =");
    ALL(a.node_words = INT64_MAX, "node_words =");
    ALL(a.C = 65, "leaf_words =");
    ALL(a.C = 257; a.leaf_words = 272, "node_words =");
    ALL(a.leaf = P(4 * U + 2), "leaf pointer");
    ALL(a.node = P(5 * U + 4), "node pointer");
    ALL(a.leaf = P(UINTPTR_MAX - 15), "address space");
    ALL(a.node = P(UINTPTR_MAX - 15), "address space");

    /* ---- insert ---- */
    INS(a.qmax = NULL, "qmax pointer is NULL");
    INS(a.K = 0, "K =");
    INS(a.K = INT64_MIN, "K =");
    INS(a.N = 0, "N =");
    INS(a.N = -5, "N =");
    INS(a.K = 9, "exceed C");
    INS(a.K = INT64_MAX; a.N = INT64_MAX, "exceed C");
    INS(a.K = (int64_t)1 << 32; a.N = (int64_t)1 << 32, "exceed C"); /* the product wraps to 0 */
    INS(a.count = ((uint64_t)1 << 63) + 1, "count =");
    INS(a.count = UINT64_MAX, "count =");
    INS(a.state_dev = P(3 * U + 4), "state_dev pointer");
    INS(a.qmax = P(6 * U + 2), "qmax pointer");
    INS(a.state_dev = P(UINTPTR_MAX - 7), "address space");
    INS(a.leaf = P(3 * U - 252), "leaf overlaps state_dev");
    INS(a.node = P(3 * U + 8), "node overlaps state_dev");
    INS(a.leaf = P(6 * U - 252), "leaf overlaps the qmax");
    INS(a.node = P(6 * U), "node overlaps the qmax");
    INS(a.node = P(4 * U + 248), "outputs leaf and node overlap");
    INS(a.count = (uint64_t)1 << 63; a.node = P(4 * U), "outputs leaf and node overlap"); /* 2^63 itself is accepted */

    /* ---- update ---- */
    UPD(a.indices = NULL, "indices pointer is NULL");
    UPD(a.td = NULL, "td_error pointer is NULL");
    UPD(a.qmax = NULL, "qmax pointer is NULL");
    UPD(a.workspace = NULL, "workspace pointer is NULL");
    UPD(a.workspace = P(12 * U + 2), "workspace pointer");
    UPD(a.workspace = P(UINTPTR_MAX - 15), "address space");
    UPD(a.workspace = P(U + 124), "workspace overlaps the indices");
    UPD(a.workspace = P(2 * U - 60), "workspace overlaps the td_error");
    UPD(a.workspace = P(5 * U + 252), "outputs node and workspace overlap");
    UPD(a.workspace = P(6 * U - 60), "outputs qmax and workspace overlap");
    UPD(a.B = 0, "B =");
    UPD(a.B = INT64_MIN, "B =");
    UPD(a.B = ((int64_t)1 << 40) + 1, "beyond 2^40 elements");
    UPD(a.B = INT64_MAX, "beyond 2^40 elements");
    UPD(a.alpha = -0.001, "alpha =");
    UPD(a.alpha = 1.001, "alpha =");
    UPD(a.alpha = NAN, "alpha =");
    UPD(a.alpha = INFINITY, "alpha =");
    UPD(a.eps = 0.0, "eps =");
    UPD(a.eps = ldexp(1.0, -65), "eps =");
    UPD(a.eps = 1.5, "eps =");
    UPD(a.eps = NAN, "eps =");
    UPD(a.eps = -1e-6, "eps =");
    UPD(a.count = ((uint64_t)1 << 63) + 1, "count =");
    UPD(a.indices = P(U + 4), "indices pointer");
    UPD(a.td = P(2 * U + 2), "td_error pointer");
    UPD(a.state_dev = P(3 * U + 4), "state_dev pointer");
    UPD(a.qmax = P(6 * U + 1), "qmax pointer");
    UPD(a.indices = P(UINTPTR_MAX - 15), "address space");
    UPD(a.td = P(UINTPTR_MAX - 7), "address space");
    UPD(a.leaf = P(U + 124), "leaf overlaps the indices");
    UPD(a.node = P(2 * U - 8), "node overlaps the td_error");
    UPD(a.qmax = P(2 * U + 60), "qmax overlaps the td_error");
    UPD(a.qmax = P(3 * U + 12), "qmax overlaps state_dev");
    UPD(a.node = P(4 * U - 248), "outputs leaf and node overlap");
    UPD(a.qmax = P(4 * U + 252), "outputs leaf and qmax overlap");
    UPD(a.qmax = P(5 * U), "outputs node and qmax overlap");
    UPD(a.eps = ldexp(1.0, -64); a.alpha = 1.0; a.qmax = P(5 * U), "outputs node and qmax overlap"); /* the bounds themselves are accepted */
    UPD(a.eps = 1.0; a.alpha = 0.0; a.qmax = P(5 * U), "outputs node and qmax overlap");

    /* ---- sample ---- */
    SMP(a.ring_obs = NULL, "ring_obs pointer is NULL");
    SMP(a.ring_next = NULL, "ring_next pointer is NULL");
    SMP(a.ring_action = NULL, "ring_action pointer is NULL");
    SMP(a.ring_reward = NULL, "ring_reward pointer is NULL");
    SMP(a.ring_term = NULL, "ring_term pointer is NULL");
    SMP(a.workspace = NULL, "workspace pointer is NULL");
    SMP(a.indices_out = NULL, "indices pointer is NULL");
    SMP(a.obs_out = NULL, "obs_out pointer is NULL");
    SMP(a.next_out = NULL, "next_out pointer is NULL");
    SMP(a.action_out = NULL, "action_out pointer is NULL");
    SMP(a.reward_out = NULL, "reward_out pointer is NULL");
    SMP(a.term_out = NULL, "term_out pointer is NULL");
    SMP(a.weights_out = NULL, "weights_out pointer is NULL");
    SMP(a.W = 0, "W =");
    SMP(a.W = -3, "W =");
    SMP(a.W = 65537, "W =");
    SMP(a.W = INT32_MAX, "W =");
    SMP(a.C = cap; a.leaf_words = cap; a.node_words = (cap >> 4) + (cap >> 8) + (cap >> 12) + (cap >> 16) + (cap >> 20) + (cap >> 24) + 32; a.W = 1024, "C * W =");
    SMP(a.B = 0, "B =");
    SMP(a.B = -7, "B =");
    SMP(a.B = ((int64_t)1 << 38) + 1, "B * W =");
    SMP(a.B = INT64_MAX, "B * W =");
    SMP(a.action_bytes = 0, "action_bytes =");
    SMP(a.action_bytes = 2, "action_bytes =");
    SMP(a.beta = -0.5, "beta =");
    SMP(a.beta = 1.0001, "beta =");
    SMP(a.beta = NAN, "beta =");
    SMP(a.ring_obs = P(7 * U + 2), "ring_obs pointer");
    SMP(a.ring_reward = P(10 * U + 3), "ring_reward pointer");
    SMP(a.workspace = P(12 * U + 2), "workspace pointer");
    SMP(a.step_dev = P(20 * U + 4), "step_dev pointer");
    SMP(a.indices_out = P(13 * U + 4), "indices pointer");
    SMP(a.obs_out = P(14 * U + 2), "obs_out pointer");
    SMP(a.action_out = P(16 * U + 4), "action_out pointer");
    SMP(a.weights_out = P(19 * U + 2), "weights_out pointer");
    SMP(a.ring_term = P(UINTPTR_MAX - 7), "address space");
    SMP(a.workspace = P(UINTPTR_MAX - 15), "address space");
    SMP(a.weights_out = P(UINTPTR_MAX - 7), "address space");
    SMP(a.step_dev = P(UINTPTR_MAX - 7), "address space");
    SMP(a.workspace = P(4 * U + 252), "workspace overlaps the leaf");
    SMP(a.indices_out = P(5 * U - 120), "indices overlaps the node");
    SMP(a.obs_out = P(8 * U - 252), "obs_out overlaps the ring_next");
    SMP(a.weights_out = P(11 * U + 60), "weights_out overlaps the ring_term");
    SMP(a.weights_out = P(20 * U + 4), "weights_out overlaps step_dev");
    SMP(a.term_out = P(20 * U - 15), "term_out overlaps step_dev");
    SMP(a.indices_out = P(12 * U + 8184), "outputs workspace and indices overlap");
    SMP(a.obs_out = P(13 * U + 120), "outputs indices and obs_out overlap");
    SMP(a.next_out = P(14 * U + 252), "outputs obs_out and next_out overlap");
    SMP(a.weights_out = P(17 * U + 60), "outputs reward_out and weights_out overlap");
    SMP(a.weights_out = P(18 * U + 12), "outputs term_out and weights_out overlap");
    SMP(a.weights_out = P(13 * U), "outputs indices and weights_out overlap");
    SMP(a.beta = 1.0; a.weights_out = P(13 * U), "outputs indices and weights_out overlap"); /* the bounds themselves are accepted */
    SMP(a.beta = 0.0; a.step_dev = NULL; a.weights_out = P(13 * U), "outputs indices and weights_out overlap");

    /* the slot is this header's own: a refusal of a uniform replay call lands in mxv_replay_last_error and leaves this one alone */
    ++calls;
    if (mxv_replay_sample(NULL, 0, 4, 16, P(U), P(U), P(U), (const float *)P(U), (const uint8_t *)P(U), 0, 0, 0, NULL, (int64_t *)P(U), P(U), P(U), P(U), 4,
                          (float *)P(U), (uint8_t *)P(U)) != MXV_ERR_INVALID_ARG ||
        !strstr(mxv_replay_last_error(), "mxv_replay_sample") || !strstr(mxv_prio_last_error(), PS)) {
        ++bad;
        printf("BAD: the two headers' error slots are not separate: '%s' / '%s'\n", mxv_replay_last_error(), mxv_prio_last_error());
    }
    printf("prio_args: calls=%d bad=%d\n", calls, bad);
    return bad != 0;
}
