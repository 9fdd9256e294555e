// mxv_prio.hip — prioritised replay on the device: the exact integer sum tree over the slots of a replay ring, its insert and update, and
// the Philox-keyed proportional draw with the gather and the importance weights (include/mxv_prio.h).
//
// Leaves are uint32, inner nodes uint64 sums; every change of a leaf travels up as an integer delta added with a no-return atomic, so the
// tree has the same bits whatever the arrival order.  Only integer atomics (32-bit exchange / max, 64-bit add), no float atomic, no
// assembly.  The float64 arithmetic — the quantisation of a TD error, the importance weight — is LOG and EXP of mxv_policy_rule.hpp.
// The results are defined bit for bit by the rule in the header (tests/prio_host.py).  The argument checks are those of
// mxv_policy_host.hpp, the row copiers those of mxv_replay_rows.hpp.
//
// Shape of the kernels (workgroups of 256 striding over tiles of 256 rows, one lane per row):
//   * add_up — a lane's delta to every ancestor of its slot.  The three levels at the top (1 + 16 + 256 nodes at most: one, one and
//     sixteen cache lines that every row of every launch hits) are summed in LDS by the workgroup over all of its tiles and added once at
//     its end; the kernels that write the tree run at most 256 workgroups for that.  Below them an insert — consecutive lanes, consecutive
//     slots — sums the lanes of a wave that hit the same node by a segmented scan and issues one add per run; an update issues one add
//     per lane, spread over at least 4096 nodes.
//   * prio_insert — leaf = *qmax_dev, delta = q - old leaf (a plain load: the slots of one launch are distinct).
//   * prio_clear, prio_raise — the two launches of an update: exchange the leaf for 0 and keep what it held beside the row; then an
//     atomic max with q, and the ancestors receive what the leaf rose by less what the row's exchange took: one trip up the tree per row,
//     not two.  prio_raise also raises *qmax_dev, once per wave and only above what it reads.
//   * prio_draw — one lane per draw: H dependent rounds, each one aligned line of 16 children (128 bytes of nodes, 64 of leaves) fetched
//     as 16-byte loads and scanned in registers.  A workgroup leaves the minimum of its drawn leaves in workspace[blockIdx.x].
//   * prio_gather_rows<WT>, prio_gather_wide<VEC> — the gather of mxv_replay.hip at the drawn slots, with the weight of each row; every
//     wave that needs it reduces the workgroup minima itself (at most 2048 words).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/mxv_prio.h"
#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"
#include "mxv_replay_rows.hpp"

namespace {

using namespace mxv::rule;
using namespace mxv::policy_host;
using namespace mxv::replay_rows;

constexpr uint32_t kStreamPrio = MXV_PRIO_STREAM_TAG;   // 1-9: mxv_device.hpp (kStream*), mxv_tab.hip, mxv_bj.hip, mxv_policy.hip, mxv_gaussian.hip, mxv_replay.hip
constexpr int kFan = MXV_PRIO_FANOUT;
constexpr int kFanBits = 4;
constexpr int kMaxLevels = 8;        // C <= 2^31: 2^27, 2^23, 2^19, 2^15, 2^11, 2^7, 8, 1
constexpr uint32_t kQMax = (uint32_t)MXV_PRIO_QMAX;
constexpr double kScale = (double)(1 << MXV_PRIO_FRAC_BITS);
constexpr double kTwo128 = 0x1p128;
constexpr int64_t kMaxCapacity = (int64_t)1 << 31;
constexpr uint64_t kMaxCount = (uint64_t)1 << 63;
constexpr int kMaxWidth = 65536;
constexpr int kTopLevels = 3;                        // levels summed in LDS: the root, 16 nodes, 256 nodes
constexpr int kTopWords = 1 + kFan + kFan * kFan;
constexpr int kTreeBlocks = 256;                     // workgroups of a kernel that writes the tree: each adds its top words once
static_assert(kFan == 1 << kFanBits && MXV_PRIO_WORKSPACE_WORDS == kMaxBlocks, "the layout and the workspace follow the launch shape");

struct Tree {
    uint32_t *leaf;
    uint64_t *node;
    int64_t off[kMaxLevels + 1];     // off[l], l = 1..H: the first word of level l in node
    int64_t C;
    int32_t H;
};

struct InsertArgs {
    Tree tree;
    const uint64_t *state_dev;
    const uint32_t *qmax;
    uint64_t count;
    int64_t R, tiles;
};

struct UpdateArgs {
    Tree tree;
    const uint64_t *state_dev;
    const int64_t *indices;
    const float *td;
    uint32_t *qmax, *saved;          // saved: what the first launch of an update took out of each row's leaf
    double alpha, eps;
    uint64_t count;
    int64_t B, tiles;
};

struct SampleArgs {
    Tree tree;
    const uint32_t *ring_obs, *ring_next, *ring_action, *ring_reward;
    const uint8_t *ring_term;
    const uint64_t *step_dev;
    uint32_t *workspace;
    int64_t *indices;
    uint32_t *obs_out, *next_out, *reward_out;
    void *action_out;
    uint8_t *term_out;
    float *weights;
    double beta;
    uint64_t seed, step;
    int64_t B, tiles;
    int32_t W, a64, minima;          // minima: the workgroups of the draw, each of which left one word in workspace
};

// ---- the rule's pieces ----
// A call, not inlined: inlined into the tile loop of prio_raise, the 26 polynomial coefficients are hoisted into scalar registers for the
// whole kernel and two of them spill.
__device__ __noinline__ uint32_t quantise(float td, double alpha, double eps) {
    const double x = (double)__builtin_fabsf(td) + eps;
    const bool finite = x < kTwo128;                    // false for NaN and +-Inf
    const double e = alpha * log_rule(finite ? x : 1.0);
    const bool small = e < 80.0;
    const double s = __builtin_rint(exp_rule(small ? e : 0.0) * kScale);
    const uint32_t q = s >= 4294967295.0 ? kQMax : s < 1.0 ? 1u : (uint32_t)s;
    return finite && small ? q : kQMax;
}

__device__ __forceinline__ float weight_of(double beta, double log_min, uint32_t q) {
    return (float)exp_rule(beta * (log_min - log_rule((double)q)));
}

// The three levels at the top of the tree — the root, the at most 16 nodes below it, the at most 256 below those — are summed in LDS
// by the whole workgroup over all of its tiles and flushed once: words 0, 1.., 17.. of `top`.
__device__ __forceinline__ int top_word(int below_root, long long node) {
    return below_root == 0 ? 0 : below_root == 1 ? 1 + (int)node : 1 + kFan + (int)node;
}
__device__ __forceinline__ void top_clear(unsigned long long *top) {
    for (int e = threadIdx.x; e < kTopWords; e += kThreads) top[e] = 0ull;
    __syncthreads();
}
__device__ __forceinline__ void top_flush(const Tree &t, const unsigned long long *top) {
    __syncthreads();
    for (int e = threadIdx.x; e < kTopWords; e += kThreads) {
        const unsigned long long sum = top[e];
        const int below_root = e == 0 ? 0 : e < 1 + kFan ? 1 : 2;
        const int l = t.H - below_root;
        if (sum != 0ull && l >= 1) atomicAdd(reinterpret_cast<unsigned long long *>(t.node + t.off[l] + (e - top_word(below_root, 0))), sum);
    }
}

// `delta` to every ancestor of slot k (k < 0: a lane without a row, delta 0).  Every lane of the wave calls this together.  The top
// levels go to LDS.  Below them, SORTED (an insert: consecutive lanes hold consecutive slots): the lanes of a wave that stand next to
// each other and hit the same node are summed by a segmented scan and the last lane of each run issues one add; otherwise (an update:
// any indices) every lane issues its own, spread over at least 4096 nodes.
template <bool SORTED>
__device__ __forceinline__ void add_up(const Tree &t, unsigned long long *top, int64_t k, uint64_t delta) {
    const int lane = threadIdx.x & 63;
    const bool mine = k >= 0 && delta != 0ull;
    for (int l = 1; l <= t.H; ++l) {
        const long long node = (long long)(k >> (kFanBits * l));     // arithmetic shift: -1 stays -1
        if (t.H - l < kTopLevels) {      // uniform
            if (mine) atomicAdd(&top[top_word(t.H - l, node)], (unsigned long long)delta);
            continue;
        }
        unsigned long long *word = reinterpret_cast<unsigned long long *>(t.node + t.off[l] + node);
        if constexpr (SORTED) {
            const long long before = __shfl_up(node, 1);
            const unsigned long long heads = __ballot(lane == 0 || before != node);
            unsigned long long sum = delta;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {     // sum over the run of equal nodes that ends at this lane
                const unsigned long long other = __shfl_up(sum, d);
                const bool same = lane >= d && ((heads >> ((lane - d + 1) & 63)) & ((1ull << d) - 1ull)) == 0;
                sum += same ? other : 0ull;
            }
            const bool last = lane == 63 || ((heads >> ((lane + 1) & 63)) & 1ull);
            if (last && sum != 0ull) atomicAdd(word, sum);
        } else {
            if (mine) atomicAdd(word, (unsigned long long)delta);
        }
    }
}

__device__ __forceinline__ uint32_t wave_min(uint32_t m) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)m, d);
        m = o < m ? o : m;
    }
    return m;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t m) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)m, d);
        m = o > m ? o : m;
    }
    return m;
}

// ---- insert ----
__global__ void __launch_bounds__(kThreads) prio_insert(const InsertArgs p) {
    __shared__ unsigned long long top[kTopWords];
    top_clear(top);
    const uint64_t c = p.state_dev ? p.state_dev[0] : p.count;
    const uint64_t s0 = c % (uint64_t)p.tree.C;
    const uint32_t q = *p.qmax;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t r = tile * kThreads + threadIdx.x;
        const bool row = r < p.R;
        const uint64_t s1 = s0 + (uint64_t)r;
        const int64_t s = row ? (int64_t)(s1 >= (uint64_t)p.tree.C ? s1 - (uint64_t)p.tree.C : s1) : -1;      // r < R <= C
        uint32_t old = q;
        if (row) {
            old = p.tree.leaf[s];
            p.tree.leaf[s] = q;
        }
        add_up<true>(p.tree, top, s, (uint64_t)q - (uint64_t)old);
    }
    top_flush(p.tree, top);
}

// ---- update ----
// min(c, C): the slots that hold a row
__device__ __forceinline__ int64_t live_slots(const UpdateArgs &p) {
    const uint64_t c = p.state_dev ? p.state_dev[0] : p.count;
    return c < (uint64_t)p.tree.C ? (int64_t)c : p.tree.C;
}
// k of row j, or -1 where the row is skipped
__device__ __forceinline__ int64_t slot_of(const UpdateArgs &p, int64_t live, int64_t j) {
    const int64_t k = j < p.B ? p.indices[j] : -1;
    return k >= 0 && k < live ? k : -1;
}

// The first launch of an update: the leaf is exchanged for 0 and what it held is kept beside the row (only the first arrival at a slot
// sees a non-zero leaf).  Nothing is added to the tree yet.
__global__ void __launch_bounds__(kThreads) prio_clear(const UpdateArgs p) {
    const int64_t live = live_slots(p);
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t j = tile * kThreads + threadIdx.x;
        if (j >= p.B) continue;
        const int64_t k = slot_of(p, live, j);
        p.saved[j] = k >= 0 ? atomicExch(&p.tree.leaf[k], 0u) : 0u;
    }
}

// The second: the leaf rises to q by an atomic max, and the ancestors receive what it rose by less what the row's exchange took away.
// Over the rows of a slot the rises telescope to the final leaf and the exchanges sum to the old one.
__global__ void __launch_bounds__(kThreads) prio_raise(const UpdateArgs p) {
    __shared__ unsigned long long top[kTopWords];
    top_clear(top);
    uint32_t best = 0u;
    const int64_t live = live_slots(p);
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t j = tile * kThreads + threadIdx.x;
        const int64_t k = slot_of(p, live, j);
        const uint32_t q = quantise(j < p.B ? p.td[j] : 0.0f, p.alpha, p.eps);
        uint32_t old = q, taken = 0u;
        if (k >= 0) {
            taken = p.saved[j];
            old = atomicMax(&p.tree.leaf[k], q);
            best = q > best ? q : best;
        }
        add_up<false>(p.tree, top, k, (uint64_t)(old > q ? old : q) - (uint64_t)old - (uint64_t)taken);
    }
    top_flush(p.tree, top);
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0 && best > *p.qmax) atomicMax(p.qmax, best);      // *qmax only grows: a stale read costs an add, never a miss
}

// ---- sample ----
// the smallest i of 16 children whose inclusive prefix sum exceeds u; u becomes what is left inside it, q the child's value
template <typename T>
__device__ __forceinline__ int pick_child(const T (&c)[kFan], uint64_t &u, uint64_t &q) {
    uint64_t acc = 0, before = 0;
    int sel = 0;
    bool found = false;
    q = 0;
#pragma unroll
    for (int i = 0; i < kFan; ++i) {
        const uint64_t next = acc + (uint64_t)c[i];
        const bool hit = !found && next > u;
        sel = hit ? i : sel;
        before = hit ? acc : before;
        q = hit ? (uint64_t)c[i] : q;
        found = found || hit;
        acc = next;
    }
    u -= before;
    return sel;
}

__device__ __forceinline__ int64_t draw(const SampleArgs &p, uint64_t t, uint64_t total, int64_t j, uint32_t &q_out) {
    const uint64_t g = (uint64_t)j >> 1;
    mxv::U4 ctr;
    ctr.x = (uint32_t)g;
    ctr.y = (uint32_t)(g >> 32);
    ctr.z = (uint32_t)t;
    ctr.w = ((uint32_t)(t >> 32) & 0x0fffffffu) | (kStreamPrio << 28);
    const mxv::U4 w4 = mxv::philox4x32_10(ctr, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
    const bool odd = ((uint32_t)j & 1u) != 0;
    const uint64_t u64 = ((uint64_t)(odd ? w4.w : w4.y) << 32) | (uint64_t)(odd ? w4.z : w4.x);
    uint64_t u = __umul64hi(u64, total), q;
    int64_t i = 0;
    for (int l = p.tree.H - 1; l >= 1; --l) {
        const ulonglong2 *line = reinterpret_cast<const ulonglong2 *>(p.tree.node + p.tree.off[l] + i * kFan);
        uint64_t c[kFan];
#pragma unroll
        for (int v = 0; v < kFan / 2; ++v) {
            const ulonglong2 x = line[v];
            c[2 * v] = x.x;
            c[2 * v + 1] = x.y;
        }
        i = i * kFan + pick_child(c, u, q);
    }
    const uint4 *line = reinterpret_cast<const uint4 *>(p.tree.leaf + i * kFan);
    uint32_t c[kFan];
#pragma unroll
    for (int v = 0; v < kFan / 4; ++v) {
        const uint4 x = line[v];
        c[4 * v] = x.x;
        c[4 * v + 1] = x.y;
        c[4 * v + 2] = x.z;
        c[4 * v + 3] = x.w;
    }
    const int64_t k = i * kFan + pick_child(c, u, q);
    q_out = (uint32_t)q;
    return k < p.tree.C ? k : p.tree.C - 1;      // a tree that holds its invariant never gets here with k >= C: memory safety only
}

__global__ void __launch_bounds__(kThreads) prio_draw(const SampleArgs p) {
    __shared__ uint32_t wave_minimum[kThreads / 64];
    const uint64_t total = p.tree.node[p.tree.off[p.tree.H]];
    const uint64_t t = p.step_dev ? p.step_dev[0] : p.step;
    uint32_t m = kQMax;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t j = tile * kThreads + threadIdx.x;
        if (j >= p.B) continue;
        int64_t k = -1;
        if (total != 0) {      // uniform
            uint32_t q;
            k = draw(p, t, total, j, q);
            m = q < m ? q : m;
        }
        p.indices[j] = k;
    }
    m = wave_min(m);
    if ((threadIdx.x & 63) == 0) wave_minimum[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) m = wave_minimum[w] < m ? wave_minimum[w] : m;
        p.workspace[blockIdx.x] = m;
    }
}

// LOG of the batch's smallest drawn leaf; every lane of the wave calls this together
__device__ __forceinline__ double log_of_minimum(const SampleArgs &p) {
    uint32_t m = kQMax;
    for (int i = threadIdx.x & 63; i < p.minima; i += 64) {
        const uint32_t x = p.workspace[i];
        m = x < m ? x : m;
    }
    return log_rule((double)wave_min(m));
}

__device__ __forceinline__ void gather_scalars(const SampleArgs &p, int64_t j, int64_t k, bool live, double log_min) {
    const uint32_t a = live ? p.ring_action[k] : 0u;
    if (p.a64) static_cast<int64_t *>(p.action_out)[j] = (int64_t)(int32_t)a;
    else static_cast<uint32_t *>(p.action_out)[j] = a;
    p.reward_out[j] = live ? p.ring_reward[k] : 0u;
    p.term_out[j] = live ? p.ring_term[k] : (uint8_t)0;
    p.weights[j] = live ? weight_of(p.beta, log_min, p.tree.leaf[k]) : 0.0f;
}

template <int WT>
__global__ void __launch_bounds__(kThreads) prio_gather_rows(const SampleArgs p) {
    const int W = WT > 0 ? WT : p.W;
    const bool live = p.tree.node[p.tree.off[p.tree.H]] != 0;      // uniform
    const double log_min = log_of_minimum(p);
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t j = tile * kThreads + threadIdx.x;
        if (j >= p.B) continue;
        const int64_t k = live ? p.indices[j] : 0;
        copy_rows<WT>(p.obs_out + j * W, p.ring_obs + k * W, p.next_out + j * W, p.ring_next + k * W, W, live);
        gather_scalars(p, j, k, live, log_min);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) prio_gather_wide(const SampleArgs p) {
    const int piece = blockIdx.x;
    const bool live = p.tree.node[p.tree.off[p.tree.H]] != 0;      // uniform
    const bool scalars = piece == 0 && threadIdx.x < 64;           // the first wave of piece 0 writes the row's scalars
    const double log_min = scalars ? log_of_minimum(p) : 0.0;
    for (int64_t j = blockIdx.y; j < p.B; j += gridDim.y) {      // j, and so k, is the workgroup's
        const int64_t k = live ? p.indices[j] : 0;
        copy_pieces<VEC>(p.obs_out + j * p.W, live ? p.ring_obs + k * p.W : nullptr, p.next_out + j * p.W, live ? p.ring_next + k * p.W : nullptr,
                         p.W, piece);
        if (scalars && threadIdx.x == 0) gather_scalars(p, j, k, live, log_min);
    }
}

// ---- host ----
using PCall = Call<mxv::PrioCall>;

int64_t tree_blocks(int64_t tiles) { return tiles < kTreeBlocks ? tiles : kTreeBlocks; }

int64_t padded(int64_t n) { return (n + kFan - 1) / kFan * kFan; }

struct Layout {
    int64_t leaf_words, node_words, off[kMaxLevels + 1];
    int32_t H;
};
Layout layout_of(int64_t C) {      // 1 <= C <= 2^31
    Layout L{};
    L.leaf_words = padded(C);
    int64_t n = C;
    do {
        n = (n + kFan - 1) / kFan;
        L.off[++L.H] = L.node_words;
        L.node_words += padded(n);
    } while (n > 1);
    return L;
}

template <int WT> struct GatherRows { static const void *ptr() { return reinterpret_cast<const void *>(&prio_gather_rows<WT>); } };
const void *pick_rows(int32_t W, bool aligned) {
    if (!aligned) return GatherRows<0>::ptr();
    switch (W) {
        case 2: return GatherRows<2>::ptr();
        case 3: return GatherRows<3>::ptr();
        case 4: return GatherRows<4>::ptr();
        case 6: return GatherRows<6>::ptr();
        default: return GatherRows<0>::ptr();
    }
}

// C, the tree's pointers and sizes; fills `tree`
int check_tree(const PCall &call, int64_t C, const uint32_t *leaf, int64_t leaf_words, const uint64_t *node, int64_t node_words, Tree &tree) {
    if (!leaf) return call.bad("%s: leaf pointer is NULL", call.api);
    if (!node) return call.bad("%s: node pointer is NULL", call.api);
    if (C < 1 || C > kMaxCapacity) return call.bad("%s: C = %lld must be in 1..2^31", call.api, (long long)C);
    const Layout L = layout_of(C);
    if (leaf_words != L.leaf_words)
        return call.bad("%s: leaf_words = %lld is not mxv_prio_layout's %lld for C = %lld", call.api, (long long)leaf_words, (long long)L.leaf_words, (long long)C);
    if (node_words != L.node_words)
        return call.bad("%s: node_words = %lld is not mxv_prio_layout's %lld for C = %lld", call.api, (long long)node_words, (long long)L.node_words, (long long)C);
    tree.leaf = const_cast<uint32_t *>(leaf);
    tree.node = const_cast<uint64_t *>(node);
    for (int l = 0; l <= kMaxLevels; ++l) tree.off[l] = L.off[l];
    tree.C = C;
    tree.H = L.H;
    return MXV_OK;
}

int check_unit(const PCall &call, const char *name, double v) {
    if (!(v >= 0.0 && v <= 1.0)) return call.bad("%s: %s = %g must be in 0..1", call.api, name, v);
    return MXV_OK;
}

}  // namespace

extern "C" {

int mxv_prio_layout(int64_t C, int64_t *leaf_words, int64_t *node_words, int32_t *levels) {
    const PCall call{"mxv_prio_layout", 'C'};
    if (C < 1 || C > kMaxCapacity) return call.bad("%s: C = %lld must be in 1..2^31", call.api, (long long)C);
    const Layout L = layout_of(C);
    if (leaf_words) *leaf_words = L.leaf_words;
    if (node_words) *node_words = L.node_words;
    if (levels) *levels = L.H;
    return MXV_OK;
}

int mxv_prio_insert(void *stream, int64_t C, int64_t K, int64_t N, uint64_t count, const uint64_t *state_dev, uint32_t *leaf_dev,
                    int64_t leaf_words, uint64_t *node_dev, int64_t node_words, const uint32_t *qmax_dev) {
    const PCall call{"mxv_prio_insert", 'n'};
    InsertArgs p{};
    if (!qmax_dev) return call.bad("%s: qmax pointer is NULL", call.api);
    if (int rc = check_tree(call, C, leaf_dev, leaf_words, node_dev, node_words, p.tree)) return rc;
    if (K < 1) return call.bad("%s: K = %lld must be at least 1", call.api, (long long)K);
    if (N < 1) return call.bad("%s: N = %lld must be at least 1", call.api, (long long)N);
    if (K > C / N) return call.bad("%s: K * N = %lld * %lld rows exceed C = %lld: two rows of one launch would share a slot", call.api, (long long)K, (long long)N, (long long)C);
    if (count > kMaxCount) return call.bad("%s: count = %llu is above 2^63", call.api, (unsigned long long)count);
    const int64_t R = K * N;
    const Range ins[] = {{"state_dev", (uintptr_t)state_dev, 16, 8, ""}, {"qmax", (uintptr_t)qmax_dev, 4, 4}};
    const Range outs[] = {{"leaf", (uintptr_t)leaf_dev, (uint64_t)leaf_words * 4, 4}, {"node", (uintptr_t)node_dev, (uint64_t)node_words * 8, 8}};
    if (int rc = call.check_ranges(R, ins, 2, outs, 2)) return rc;
    p.state_dev = state_dev; p.qmax = qmax_dev; p.count = count; p.R = R; p.tiles = (R + kThreads - 1) / kThreads;
    return call.launch_blocks(reinterpret_cast<const void *>(&prio_insert), p, tree_blocks(p.tiles), stream);
}

int mxv_prio_update(void *stream, int64_t C, int64_t B, const int64_t *indices_dev, const float *td_error_dev, double alpha, double eps,
                    uint64_t count, const uint64_t *state_dev, uint32_t *leaf_dev, int64_t leaf_words, uint64_t *node_dev,
                    int64_t node_words, uint32_t *qmax_dev, uint32_t *workspace_dev) {
    const PCall call{"mxv_prio_update", 'B'};
    UpdateArgs p{};
    if (!indices_dev) return call.bad("%s: indices pointer is NULL", call.api);
    if (!td_error_dev) return call.bad("%s: td_error pointer is NULL", call.api);
    if (!qmax_dev) return call.bad("%s: qmax pointer is NULL", call.api);
    if (!workspace_dev) return call.bad("%s: workspace pointer is NULL", call.api);
    if (int rc = check_tree(call, C, leaf_dev, leaf_words, node_dev, node_words, p.tree)) return rc;
    if (B < 1) return call.bad("%s: B = %lld must be at least 1", call.api, (long long)B);
    if (int rc = call.check_stride(1, B)) return rc;
    if (int rc = check_unit(call, "alpha", alpha)) return rc;
    if (!(eps >= 0x1p-64 && eps <= 1.0)) return call.bad("%s: eps = %g must be in 2^-64..1", call.api, eps);
    if (count > kMaxCount) return call.bad("%s: count = %llu is above 2^63", call.api, (unsigned long long)count);
    const Range ins[] = {{"indices", (uintptr_t)indices_dev, (uint64_t)B * 8, 8}, {"td_error", (uintptr_t)td_error_dev, (uint64_t)B * 4, 4},
                         {"state_dev", (uintptr_t)state_dev, 16, 8, ""}};
    const Range outs[] = {{"leaf", (uintptr_t)leaf_dev, (uint64_t)leaf_words * 4, 4}, {"node", (uintptr_t)node_dev, (uint64_t)node_words * 8, 8},
                          {"qmax", (uintptr_t)qmax_dev, 4, 4}, {"workspace", (uintptr_t)workspace_dev, (uint64_t)B * 4, 4}};
    if (int rc = call.check_ranges(B, ins, 3, outs, 4)) return rc;
    p.state_dev = state_dev; p.indices = indices_dev; p.td = td_error_dev; p.qmax = qmax_dev; p.saved = workspace_dev; p.alpha = alpha; p.eps = eps; p.count = count;
    p.B = B; p.tiles = (B + kThreads - 1) / kThreads;
    if (int rc = call.launch(reinterpret_cast<const void *>(&prio_clear), p, stream)) return rc;
    return call.launch_blocks(reinterpret_cast<const void *>(&prio_raise), p, tree_blocks(p.tiles), stream);
}

int mxv_prio_sample(void *stream, int64_t C, int32_t W, int64_t B, const void *ring_obs_dev, const void *ring_next_dev,
                    const void *ring_action_dev, const float *ring_reward_dev, const uint8_t *ring_term_dev, const uint32_t *leaf_dev,
                    int64_t leaf_words, const uint64_t *node_dev, int64_t node_words, uint64_t seed, uint64_t step, uint64_t *step_dev,
                    double beta, uint32_t *workspace_dev, int64_t *indices_dev, void *obs_out_dev, void *next_out_dev,
                    void *action_out_dev, int32_t action_bytes, float *reward_out_dev, uint8_t *term_out_dev, float *weights_out_dev) {
    const PCall call{"mxv_prio_sample", 'B'};
    SampleArgs p{};
    if (!ring_obs_dev) return call.bad("%s: ring_obs pointer is NULL", call.api);
    if (!ring_next_dev) return call.bad("%s: ring_next pointer is NULL", call.api);
    if (!ring_action_dev) return call.bad("%s: ring_action pointer is NULL", call.api);
    if (!ring_reward_dev) return call.bad("%s: ring_reward pointer is NULL", call.api);
    if (!ring_term_dev) return call.bad("%s: ring_term pointer is NULL", call.api);
    if (!workspace_dev) return call.bad("%s: workspace pointer is NULL", call.api);
    if (!indices_dev) return call.bad("%s: indices pointer is NULL", call.api);
    if (!obs_out_dev) return call.bad("%s: obs_out pointer is NULL", call.api);
    if (!next_out_dev) return call.bad("%s: next_out pointer is NULL", call.api);
    if (!action_out_dev) return call.bad("%s: action_out pointer is NULL", call.api);
    if (!reward_out_dev) return call.bad("%s: reward_out pointer is NULL", call.api);
    if (!term_out_dev) return call.bad("%s: term_out pointer is NULL", call.api);
    if (!weights_out_dev) return call.bad("%s: weights_out pointer is NULL", call.api);
    if (int rc = check_tree(call, C, leaf_dev, leaf_words, node_dev, node_words, p.tree)) return rc;
    if (W < 1 || W > kMaxWidth) return call.bad("%s: W = %d must be in 1..%d", call.api, (int)W, kMaxWidth);
    if (W > kMaxElems / C) return call.bad("%s: C * W = %lld * %d is beyond 2^40 dwords", call.api, (long long)C, (int)W);
    if (B < 1) return call.bad("%s: B = %lld must be at least 1", call.api, (long long)B);
    if (B > kMaxElems / W) return call.bad("%s: B * W = %lld * %d is beyond 2^40 dwords", call.api, (long long)B, (int)W);
    if (action_bytes != 4 && action_bytes != 8) return call.bad("%s: action_bytes = %d must be 4 (int32, float32) or 8 (int64)", call.api, (int)action_bytes);
    if (int rc = check_unit(call, "beta", beta)) return rc;
    const uint64_t ab = (uint64_t)action_bytes, ring_row_bytes = (uint64_t)C * (uint64_t)W * 4, out_row_bytes = (uint64_t)B * (uint64_t)W * 4;
    const Range ins[] = {{"ring_obs", (uintptr_t)ring_obs_dev, ring_row_bytes, 4}, {"ring_next", (uintptr_t)ring_next_dev, ring_row_bytes, 4},
                         {"ring_action", (uintptr_t)ring_action_dev, (uint64_t)C * 4, 4}, {"ring_reward", (uintptr_t)ring_reward_dev, (uint64_t)C * 4, 4},
                         {"ring_term", (uintptr_t)ring_term_dev, (uint64_t)C, 1}, {"leaf", (uintptr_t)leaf_dev, (uint64_t)leaf_words * 4, 4},
                         {"node", (uintptr_t)node_dev, (uint64_t)node_words * 8, 8}, {"step_dev", (uintptr_t)step_dev, 8, 8, ""}};
    const Range outs[] = {{"workspace", (uintptr_t)workspace_dev, (uint64_t)MXV_PRIO_WORKSPACE_WORDS * 4, 4},
                          {"indices", (uintptr_t)indices_dev, (uint64_t)B * 8, 8}, {"obs_out", (uintptr_t)obs_out_dev, out_row_bytes, 4},
                          {"next_out", (uintptr_t)next_out_dev, out_row_bytes, 4}, {"action_out", (uintptr_t)action_out_dev, (uint64_t)B * ab, ab},
                          {"reward_out", (uintptr_t)reward_out_dev, (uint64_t)B * 4, 4}, {"term_out", (uintptr_t)term_out_dev, (uint64_t)B, 1},
                          {"weights_out", (uintptr_t)weights_out_dev, (uint64_t)B * 4, 4}};
    if (int rc = call.check_ranges(B, ins, 8, outs, 8)) return rc;
    p.ring_obs = static_cast<const uint32_t *>(ring_obs_dev); p.ring_next = static_cast<const uint32_t *>(ring_next_dev);
    p.ring_action = static_cast<const uint32_t *>(ring_action_dev); p.ring_reward = reinterpret_cast<const uint32_t *>(ring_reward_dev);
    p.ring_term = ring_term_dev; p.step_dev = step_dev; p.workspace = workspace_dev; p.indices = indices_dev;
    p.obs_out = static_cast<uint32_t *>(obs_out_dev); p.next_out = static_cast<uint32_t *>(next_out_dev);
    p.reward_out = reinterpret_cast<uint32_t *>(reward_out_dev); p.action_out = action_out_dev; p.term_out = term_out_dev; p.weights = weights_out_dev;
    p.beta = beta; p.seed = seed; p.step = step; p.B = B; p.tiles = (B + kThreads - 1) / kThreads; p.W = W; p.a64 = action_bytes == 8;
    p.minima = (int32_t)grid_of(p.tiles).x;
    if (int rc = call.launch(reinterpret_cast<const void *>(&prio_draw), p, stream)) return rc;
    Aligned al{wanted_alignment(W)};
    al.base(ring_obs_dev); al.base(ring_next_dev); al.base(obs_out_dev); al.base(next_out_dev); al.stride(W);
    if (W > kNarrow) {
        const void *kernel = al.ok && al.align == 16 ? reinterpret_cast<const void *>(&prio_gather_wide<true>) : reinterpret_cast<const void *>(&prio_gather_wide<false>);
        if (int rc = launch_wide(call, kernel, p, B, stream)) return rc;
    } else {
        if (int rc = call.launch(pick_rows(W, al.ok), p, stream)) return rc;
    }
    return call.advance(step_dev, stream);
}

const char *mxv_prio_last_error(void) { return mxv::last_error<mxv::PrioCall>(nullptr); }

}  // extern "C"
