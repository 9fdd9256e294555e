// mxv_replay_rows.hpp — the row copiers that the replay kernels share: mxv_replay.hip (the uniform buffer, include/mxv_replay.h) and
// mxv_prio.hip (the prioritised draws, include/mxv_prio.h) gather a transition's two observation rows with these lines, so both move a
// row in the same accesses.  Device helpers and the host's choice between them; no kernel is defined here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mxv_policy_host.hpp"
#include "mxv_policy_rule.hpp"

namespace mxv {
namespace replay_rows {

using rule::kThreads;

constexpr int kNarrow = 8;           // rows of up to this many dwords: one lane per transition
constexpr int kPiece = 1024;         // dwords of a wide row that one workgroup copies: four per lane
constexpr int kWideRows = 16384;     // gridDim.y of the wide kernels at most: workgroups stride over the rows beyond it

// alignment in bytes of a row of the straight-line instantiation WT
template <int WT>
constexpr int row_align() {
    return WT == 4 ? 16 : (WT == 2 || WT == 6) ? 8 : 4;
}

// two rows of W dwords at once (a transition's obs and next): both are read before either is written.  `live` is uniform; a row that is
// not live is written as zeros and its source is not read.
template <int WT>
__device__ __forceinline__ void copy_rows(uint32_t *dst_a, const uint32_t *src_a, uint32_t *dst_b, const uint32_t *src_b, int W, bool live) {
    if constexpr (WT > 0) {
        constexpr int kAlign = row_align<WT>();
        const uint32_t *sa = static_cast<const uint32_t *>(__builtin_assume_aligned(src_a, kAlign));
        const uint32_t *sb = static_cast<const uint32_t *>(__builtin_assume_aligned(src_b, kAlign));
        uint32_t *da = static_cast<uint32_t *>(__builtin_assume_aligned(dst_a, kAlign));
        uint32_t *db = static_cast<uint32_t *>(__builtin_assume_aligned(dst_b, kAlign));
        uint32_t x[WT], y[WT];
#pragma unroll
        for (int k = 0; k < WT; ++k) x[k] = y[k] = 0u;
        if (live) {
#pragma unroll
            for (int k = 0; k < WT; ++k) x[k] = sa[k];      // one access of WT dwords (two for WT = 6)
#pragma unroll
            for (int k = 0; k < WT; ++k) y[k] = sb[k];
        }
#pragma unroll
        for (int k = 0; k < WT; ++k) da[k] = x[k];
#pragma unroll
        for (int k = 0; k < WT; ++k) db[k] = y[k];
    } else {
        for (int k = 0; k < W; ++k) {      // keeps nothing per column
            const uint32_t x = live ? src_a[k] : 0u, y = live ? src_b[k] : 0u;
            dst_a[k] = x;
            dst_b[k] = y;
        }
    }
}

// ---- wide rows: a workgroup per (row, piece) ----
// the piece `piece` of two rows at once: both are loaded before either is stored.  A NULL source row stores zeros.
template <bool VEC>
__device__ __forceinline__ void copy_pieces(uint32_t *dst_a, const uint32_t *src_a, uint32_t *dst_b, const uint32_t *src_b, int W, int piece) {
    const int tid = threadIdx.x;
    const bool zero = src_a == nullptr;      // uniform
    if constexpr (VEC) {
        const int o = piece * kPiece + tid * 4;
        if (o >= W) return;      // W % 4 == 0: the 16 bytes lie inside the row
        uint4 x = make_uint4(0u, 0u, 0u, 0u), y = x;
        if (!zero) {
            x = *reinterpret_cast<const uint4 *>(src_a + o);
            y = *reinterpret_cast<const uint4 *>(src_b + o);
        }
        *reinterpret_cast<uint4 *>(dst_a + o) = x;
        *reinterpret_cast<uint4 *>(dst_b + o) = y;
    } else {
        constexpr int kPer = kPiece / kThreads;
        uint32_t x[kPer], y[kPer];
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int o = piece * kPiece + q * kThreads + tid;
            const bool in = o < W && !zero;
            x[q] = in ? src_a[o] : 0u;
            y[q] = in ? src_b[o] : 0u;
        }
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int o = piece * kPiece + q * kThreads + tid;
            if (o < W) {
                dst_a[o] = x[q];
                dst_b[o] = y[q];
            }
        }
    }
}

// ---- host ----
// bytes on which one access of a whole row must lie: 16 for a wide row copied in 16-byte pieces, what row_align says for a narrow one
inline uint64_t wanted_alignment(int32_t W) {
    if (W > kNarrow) return W % 4 == 0 ? 16 : 4;
    return W == 4 ? 16 : (W == 2 || W == 6) ? 8 : 4;
}
// every base given, and every stride given (in dwords), keeps `align` bytes
struct Aligned {
    uint64_t align;
    bool ok = true;
    void base(const void *p) { ok = ok && ((uintptr_t)p & (align - 1)) == 0; }
    void stride(int64_t ld) { ok = ok && (((uint64_t)ld * 4) & (align - 1)) == 0; }
};

// a wide launch: blockIdx.x the piece, blockIdx.y striding over the rows
template <class Slot, typename Args>
int launch_wide(const policy_host::Call<Slot> &call, const void *kernel, Args &a, int64_t rows, void *stream) {
    void *args[] = {&a};
    const dim3 grid((unsigned)((a.W + kPiece - 1) / kPiece), (unsigned)(rows < kWideRows ? rows : kWideRows));
    const hipError_t e = hipLaunchKernel(kernel, grid, dim3(kThreads), args, 0, (hipStream_t)stream);
    return e == hipSuccess ? MXV_OK : call.hip_failed("kernel launch", e);
}

}  // namespace replay_rows
}  // namespace mxv
