// gswm_topk.h -- running top-8 lists of int64 keys (score << 32) | (0xFFFFFFFF - index), shared by the registry searches
// (gswm_trace.hip, gswm_keyed.hip).  The maximum of a set of keys is the best score with the LOWEST index and keys are unique, so the
// k largest of any partition's k largest are the k largest overall.  The way from the lanes' lists to the answer is here as well:
// lane lists -> LDS -> one list per (workgroup, image) in the caller's workspace (workgroup_lists_to_partial) -> the k largest of an
// image's partial lists in one wave (wave_merge_partial).  Device code only; include after <hip/hip_runtime.h>.
#pragma once
#include <climits>
#include <cstdint>

namespace {

constexpr int TR_LIST = 8;               // entries of a running list (k <= 8)
constexpr int64_t TR_EMPTY = INT64_MIN;  // score INT32_MIN, index -1

// keep the 8 largest keys, L[0] the largest
__device__ __forceinline__ void list_insert(int64_t (&L)[TR_LIST], int64_t key) {
    if (key > L[TR_LIST - 1]) {
        L[TR_LIST - 1] = key;
#pragma unroll
        for (int j = TR_LIST - 1; j > 0; --j) {
            const int64_t a = L[j - 1], b = L[j];
            const bool sw = b > a;
            L[j - 1] = sw ? b : a;
            L[j] = sw ? a : b;
        }
    }
}

__device__ __forceinline__ int64_t make_key(int r1, int64_t u) {
    return (int64_t)(((uint64_t)(uint32_t)r1 << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)u));
}

// fold the list of lane ^ step into this lane's (both lanes end with the same list)
__device__ __forceinline__ void merge_from_lane_xor(int64_t (&L)[TR_LIST], int step) {
    int64_t other[TR_LIST];
#pragma unroll
    for (int j = 0; j < TR_LIST; ++j) other[j] = __shfl_xor((long long)L[j], step);
#pragma unroll
    for (int j = 0; j < TR_LIST; ++j) list_insert(L, other[j]);
}

// The end of a scan kernel, first half.  wlist is LDS, [WAVES][IMGS][TR_LIST]: the lane of wave `wave` that owns image slot i puts its list
// at slot = wave * IMGS + i; the workgroup's barrier follows.
__device__ __forceinline__ void put_list(int64_t* wlist, int slot, const int64_t (&L)[TR_LIST]) {
#pragma unroll
    for (int j = 0; j < TR_LIST; ++j) wlist[slot * TR_LIST + j] = L[j];
}

// Second half, after the barrier: thread i < IMGS merges the WAVES lists of slot i and stores the first k keys as the workgroup's list of
// image img0 + i (if that is an image: < B).  partial is [B][grid_x][k], the workgroup is blockIdx.x.
template <int WAVES, int IMGS>
__device__ __forceinline__ void workgroup_lists_to_partial(const int64_t* wlist, int img0, int B, int64_t* partial, int grid_x, int k) {
    const int tid = threadIdx.x;
    if (tid < IMGS) {
        int64_t F[TR_LIST];
#pragma unroll
        for (int j = 0; j < TR_LIST; ++j) F[j] = wlist[tid * TR_LIST + j];
        for (int w = 1; w < WAVES; ++w)
#pragma unroll
            for (int j = 0; j < TR_LIST; ++j) list_insert(F, wlist[(w * IMGS + tid) * TR_LIST + j]);
        const int b = img0 + tid;
        if (b < B) {
            int64_t* dst = partial + ((int64_t)b * grid_x + blockIdx.x) * k;
#pragma unroll
            for (int j = 0; j < TR_LIST; ++j)
                if (j < k) dst[j] = F[j];
        }
    }
}

// The start of a finish kernel, one wave per image: every lane ends with the TR_LIST largest of the n keys at src.
__device__ __forceinline__ void wave_merge_partial(int64_t (&L)[TR_LIST], const int64_t* src, int n, int lane) {
#pragma unroll
    for (int j = 0; j < TR_LIST; ++j) L[j] = TR_EMPTY;
    for (int i = lane; i < n; i += 64) list_insert(L, src[i]);
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) merge_from_lane_xor(L, step);
}

}  // namespace
