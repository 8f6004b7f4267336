// Host-only vocabulary of the mesh-side exports: what an export refuses, and its one-dimensional launch.  No device code.
// An export checks, in the order its own file states: null or misaligned pointers (MD_ERR_BAD_ARG), sizes and scalars
// (MD_ERR_BAD_ARG), limits (MD_ERR_UNSUPPORTED), aliasing (MD_ERR_BAD_ARG).  Alignment 1 means "only null is refused".
#pragma once
#include "md_common.h"

// an optional pointer: null is allowed, a misaligned address is not
template <uintptr_t A, class... P> static inline bool md_any_misaligned(const P*... p) { return ((((uintptr_t)p & (A - 1)) != 0) || ...); }
// a required pointer: null or misaligned
template <uintptr_t A, class... P> static inline bool md_any_bad(const P*... p) { return ((!p || ((uintptr_t)p & (A - 1))) || ...); }
// every count is at most INT32_MAX (the kernels index with int)
template <class... N> static inline bool md_fits_i32(N... n) { return (((int64_t)n <= 0x7fffffffLL) && ...); }
static inline unsigned md_blocks(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// The tail of an export that is one 1-D launch of `n` threads on `stream` (the export's last parameter) and nothing else.
#define MD_LAUNCH_1D(kernel, n, threads, ...)                                                                            \
  do {                                                                                                                   \
    MD_HIP_CLEAR_ERROR();                                                                                                \
    hipLaunchKernelGGL(kernel, dim3(md_blocks(n, threads)), dim3(threads), 0, (hipStream_t)stream, __VA_ARGS__);         \
    MD_HIP_CHECK_LAUNCH();                                                                                               \
    return MD_OK;                                                                                                        \
  } while (0)
