// drgnn_capi_common.h -- what more than one of the drgnn_capi*.hip units uses; included by those units and by nothing else.
// No state: a file-scope variable stays in the one unit that owns it.
#pragma once
#include "drgnn_rt.h"
#include "../../include/drgnn.h"

#include <vector>
#include <algorithm>
#include <memory>
#include <type_traits>
#include <string.h>
#include <stdlib.h>
#define DRGNN_LDS_LIMIT (160 * 1024)
#ifndef DRGNN_EMU      // (the emulation makes no runtime call)
#define HIP_TRY(expr)                                 \
    do {                                                \
        hipError_t e_ = (expr);                         \
        if (e_ != hipSuccess) return (int)e_;           \
    } while (0)
#endif
#include "drgnn_launch.h"

// ---- request checks that several entry points share -----------------------------------------------------
// the ragged layout on the host, whole, before anything is indexed through it: 0 = ap[0] <= ap[r] <= ap[r + 1], ap[R] = T;
// with rp, 0 = rp[0] <= rp[c] <= rp[c + 1] <= R = rp[M]; with sp, rp[c] <= sp[c] <= rp[c + 1]
static inline bool ragged_check(const int32_t* ap, const int32_t* rp, const int32_t* sp, int64_t T, int64_t R, int64_t M) {
    if (ap[0] != 0 || ap[R] != T || (rp && (rp[0] != 0 || rp[M] != R))) return false;
    for (int64_t r = 0; r < R; ++r)
        if (ap[r + 1] < ap[r]) return false;
    for (int64_t c = 0; rp && c < M; ++c)
        if (rp[c + 1] < rp[c] || rp[c + 1] > R || (sp && (sp[c] < rp[c] || sp[c] > rp[c + 1]))) return false;
    return true;
}

// every target (complex tc[k], residue tr[k]) lies inside its complex; rp has passed ragged_check
static inline bool targets_check(const int32_t* tc, const int32_t* tr, const int32_t* rp, int64_t M, int64_t K) {
    for (int64_t k = 0; k < K; ++k)
        if (tc[k] < 0 || tc[k] >= M || tr[k] < rp[tc[k]] || tr[k] >= rp[tc[k] + 1]) return false;
    return true;
}

// pointer first (alignment: a power of two), then the size: the workspace of depth and RMSD
static inline int workspace_check(const void* ptr, int64_t bytes, int64_t need, uintptr_t alignment) {
    if (!ptr || ((uintptr_t)ptr & (alignment - 1))) return DRGNN_E_ARG;
    return bytes < need ? DRGNN_E_CAPACITY : 0;
}

// drgnn_<subsystem>_capacity(what): entry `what` of the subsystem's limits, -1 beyond them
#define DRGNN_CAPACITY(name, ...)                                                              \
    int32_t name(int32_t what) {                                                               \
        static const int32_t cap[] = {__VA_ARGS__};                                            \
        return what >= 0 && what < (int32_t)(sizeof(cap) / sizeof(cap[0])) ? cap[what] : -1;   \
    }
