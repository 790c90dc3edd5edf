// gswm_topk.h -- running top-8 lists of int64 keys (score << 32) | (0xFFFFFFFF - index), shared by the registry searches
// (gswm_trace.hip, gswm_keyed.hip).  The maximum of a set of keys is the best score with the LOWEST index and keys are unique, so the
// k largest of any partition's k largest are the k largest overall.  Device code only; include after <hip/hip_runtime.h>.
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

}  // namespace
