// pk_libkernel.h -- private to the units whose kernels are compiled into the library itself, not into a model's code object
// (pk_ops.cpp, pk_reduce.cpp, pk_merit.cpp, pk_cg.cpp, pk_minres.cpp): what such a unit needs around its own arithmetic, stated once.
//
// A unit writes the work of one thread as PK_LIB_FN functions.  Under __HIPCC__ its kernels call them between barriers; without
// it (the CPU-only builds of tests/fake_hip) a host function walks the same work items with the same grid stride, thread by
// thread, enqueued on the stand-in's stream where the kernel would have been launched.  Nothing here does floating-point
// arithmetic: the association and the rounding of every result are the unit's own.
#ifndef PK_LIBKERNEL_H
#define PK_LIBKERNEL_H

#include "pk_runtime.h"

#ifdef __HIPCC__
#define PK_LIB_FN __host__ __device__ __forceinline__
#else
#define PK_LIB_FN inline
#endif

static_assert((PK_BLOCK & (PK_BLOCK - 1)) == 0, "the tree halves the workgroup");

// The grid rule of every library kernel: one workgroup per work item up to PK_LIB_GRID_CAP (8 workgroups of 256 threads fill a
// CU's 2048 thread slots, 256 CUs), the items beyond it in a stride loop.  A work item's result is a function of the item
// alone: it does not depend on the cap.
enum { PK_LIB_GRID_CAP = 2048 };
inline unsigned lib_grid(int64_t items) { return (unsigned)std::min<int64_t>(items, PK_LIB_GRID_CAP); }

// The fixed tree over the workgroup's LDS, widths PK_BLOCK / 2 ... 1 with a barrier behind every level.  The step is the
// unit's: step(s, w, t, more...) is what thread t does at width w (which slots, + or max, how many columns share the level).
#ifdef __HIPCC__
template <class Step, class... More>
__device__ __forceinline__ void lib_tree(Step step, double* s, int t, More... more) {      // (every thread of the workgroup)
#pragma unroll
  for (int w = PK_BLOCK / 2; w >= 1; w >>= 1) {
    step(s, w, t, more...);
    __syncthreads();
  }
}

// One statement per launch site: the kernel, its host walk (unused here), the grid, the stream, the arguments by value.
#define PK_LIB_LAUNCH(c, kernel, host_walk, grid, st, args)                      \
  do {                                                                           \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(PK_BLOCK), 0, (st), (args));     \
    PK_HIP((c), hipGetLastError());                                              \
  } while (0)
#else
template <class Step, class... More>
inline void lib_tree_host(Step step, double* s, More... more) {
  for (int w = PK_BLOCK / 2; w >= 1; w >>= 1)
    for (int t = 0; t < PK_BLOCK; ++t) step(s, w, t, more...);
}

// the work items workgroup wg of a grid takes, workgroup by workgroup: wg, wg + grid, ...
template <class Item>
inline void lib_walk_host(unsigned grid, int64_t items, Item item) {
  for (unsigned wg = 0; wg < grid; ++wg)
    for (int64_t i = wg; i < items; i += grid) item(i);
}

#define PK_LIB_LAUNCH(c, kernel, host_walk, grid, st, args) \
  fake_hip_enqueue((st), [a_ = (args), g_ = (grid)]() { host_walk(a_, g_); })
#endif

#endif  // PK_LIBKERNEL_H
