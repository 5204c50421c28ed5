// What at least two of sparse_counts.hip, sparse_linear.hip, sparse_gram.hip and expr_moments.hip use.  A matrix is a list of
// lines (sparse_counts.hip): line l owns the entries lineptr[l] .. lineptr[l + 1] of idx and val; a launch walks the lines
// `lines[row]` (a NULL list: line = row).  A NEGATIVE entry of the list is an empty line in every kernel: none of its entries is
// read, the row gets what a line without entries gets.  The pointers read for it are line 0's, so a matrix that is walked through
// such a list has at least one line: one adjacent pair keeps the walk's single 16-byte scalar load; `if (line < 0) return {0, 0}`
// and a load at lineptr[l + (line >= 0)] both cost expand's short workgroups 0.5 - 1.3 % (profiles/sparse_refactor_kbench_ab.txt).
#pragma once
#include "common.h"

constexpr long LINES_MAX = 2147483647L;          // lines of one launch: grid.x; a line list is int32 anyway

struct LineRange { int64_t b, e; };              // the line's entries [b, e)
__device__ __forceinline__ LineRange line_range(const int64_t* __restrict__ lineptr, const int32_t* __restrict__ lines, int64_t row) {
    const int64_t line = lines ? (int64_t)lines[row] : row;
    const int64_t l = line < 0 ? 0 : line;       // one adjacent pair of pointers whatever the sign: no branch, one load
    const int64_t b = lineptr[l], e = lineptr[l + 1];
    return {b, line < 0 ? b : e};
}

// lane j's value of x in every lane; j is wave-uniform
__device__ __forceinline__ int lane_get(int x, int j) { return __builtin_amdgcn_readlane(x, j); }
__device__ __forceinline__ float lane_get(float x, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j)); }
__device__ __forceinline__ int64_t lane_get(int64_t x, int j) {
    const int lo = __builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)x, j);
    const int hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)x >> 32), j);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// p is not a multiple of `to` bytes (a power of two); NULL is aligned
static inline bool lines_misaligned(const void* p, uintptr_t to = 4) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }

// The head of every launcher over n lines: the one order of the status codes.  bad, unsupported: the launcher's own conditions;
// a, b: idx and val, needed from the first line on.  LINES_GO: go on and launch; anything else is the status to return.
constexpr int LINES_GO = 1;                      // no GNX status is positive
static inline int lines_preamble(long n, const void* lineptr, bool bad, bool unsupported, const void* a, const void* b) {
    if (n < 0 || !lineptr || bad) return GNX_ERR_BAD_ARG;
    if (n > LINES_MAX || unsupported) return GNX_ERR_UNSUPPORTED;
    if (n == 0) return GNX_OK;
    if (!a || !b) return GNX_ERR_BAD_ARG;
    return LINES_GO;
}
