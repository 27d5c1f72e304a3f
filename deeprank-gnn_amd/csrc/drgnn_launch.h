// drgnn_launch.h -- the one launch form of the entry points of the drgnn_capi*.hip units, features and training path (included
// through drgnn_capi_common.h, by those units alone).
//
//     DRGNN_EMU_ONLY(std::unique_ptr<XShared> lds(new XShared);)
//     DRGNN_LAUNCH(k_x, grid1(n_blocks), stream, x_block(a, bx, *lds), a);
//
// The product build launches kernel k_x with the arguments after the body; the emulation runs the body once per workgroup, the
// block indices in scope as bx and by.  Either way the entry point's phases, guards and early returns are written once.
#pragma once

// blocks in x and y, threads of a block, bytes of dynamic LDS
struct Grid { int64_t x, y; int threads; int64_t lds; };
static inline Grid grid1(int64_t x, int threads = DRGNN_NTHREADS, int64_t lds = 0) { return Grid{x, 1, threads, lds}; }
static inline Grid grid2(int64_t x, int64_t y, int threads = DRGNN_NTHREADS) { return Grid{x, y, threads, 0}; }

#ifdef DRGNN_EMU
// what only the emulation declares: the stand-in for a kernel's shared memory
#define DRGNN_EMU_ONLY(...) __VA_ARGS__
// a kernel as a value (the emulation has no kernels: the body of the launch names the block function)
#define DRGNN_KERNEL(k) nullptr
// the item kernels (a lane per item, guarded in the kernel or its item function): the emulation's "workgroup" is one item
static inline Grid grid_items(int64_t n, int threads = 256) { return Grid{n, 1, 1, 0}; }
#define DRGNN_LAUNCH(kern, grid, stream, body, ...)                                  \
    do {                                                                             \
        const Grid g_ = (grid);                                                      \
        (void)(stream);                                                              \
        for (int64_t by = 0; by < g_.y; ++by)                                        \
            for (int64_t bx = 0; bx < g_.x; ++bx) { body; }                          \
    } while (0)
static inline int drgnn_clear(void* p, size_t bytes, void* stream) {
    (void)stream;
    if (bytes) memset(p, 0, bytes);
    return 0;
}
#else
#define DRGNN_EMU_ONLY(...)
#define DRGNN_KERNEL(k) k
static inline Grid grid_items(int64_t n, int threads = 256) { return Grid{(n + threads - 1) / threads, 1, threads, 0}; }
// An empty grid is skipped (a launch of zero blocks is an error); an error of the launch returns from the ENCLOSING function.
#define DRGNN_LAUNCH(kern, grid, stream, body, ...)                                                                      \
    do {                                                                                                                 \
        const Grid g_ = (grid);                                                                                          \
        if (g_.x > 0 && g_.y > 0) {                                                                                      \
            hipError_t e_ = hipSuccess;                                                                                  \
            if (g_.lds > 64 * 1024)                                                                                      \
                e_ = hipFuncSetAttribute((const void*)(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g_.lds);  \
            if (e_ != hipSuccess) return (int)e_;                                                                        \
            hipLaunchKernelGGL(kern, dim3((unsigned)g_.x, (unsigned)g_.y), dim3((unsigned)g_.threads), (size_t)g_.lds,   \
                               (hipStream_t)(stream), __VA_ARGS__);                                                      \
            if ((e_ = hipGetLastError()) != hipSuccess) return (int)e_;                                                  \
        }                                                                                                                \
    } while (0)
static inline int drgnn_clear(void* p, size_t bytes, void* stream) {
    return bytes ? (int)hipMemsetAsync(p, 0, bytes, (hipStream_t)stream) : 0;
}
#endif
