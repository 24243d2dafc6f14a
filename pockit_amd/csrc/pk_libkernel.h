// pk_libkernel.h -- private to the units whose kernels are compiled into the library itself, not into a model's code object
// (pk_ops.cpp, pk_reduce.cpp, pk_merit.cpp, pk_cg.cpp, pk_minres.cpp, pk_ipm.cpp, pk_slack.cpp, pk_band.cpp): what such a unit needs around its own arithmetic, stated once
// -- function macro, grid rule, tree driver, launch, host walk -- and the pieced dot the two solvers share.
//
// A unit writes the work of one thread as PK_LIB_FN functions.  Under __HIPCC__ its kernels call them between barriers; without
// it (the CPU-only builds of tests/fake_hip) a host function walks the same work items with the same grid stride, thread by
// thread, enqueued on the stand-in's stream where the kernel would have been launched.
//
// The only floating-point arithmetic here is that of the pieced dot below: the additions of its tree (lib_planes_step) and of
// the strided trip of its scalar step (lib_scalar_thread).  No product is formed here, so nothing here can contract; every
// term, its rounding and the order in which a thread adds its own terms are the unit's.  A unit still includes this header
// behind its contraction pragma.
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
// The second form, for a batch of systems behind one plan: the grid is (grid, ny); the kernel takes its entry from blockIdx.y
// and walks blockIdx.x as under the one-dimensional form.
#define PK_LIB_LAUNCH_Y(c, kernel, host_walk, grid, ny, st, args)                       \
  do {                                                                                  \
    hipLaunchKernelGGL(kernel, dim3((grid), (ny)), dim3(PK_BLOCK), 0, (st), (args));    \
    PK_HIP((c), hipGetLastError());                                                     \
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
// the second form: the entries outermost; host_walk(args, grid, y) is the one-dimensional walk of entry y
#define PK_LIB_LAUNCH_Y(c, kernel, host_walk, grid, ny, st, args)                \
  fake_hip_enqueue((st), [a_ = (args), g_ = (grid), y_ = (unsigned)(ny)]() {     \
    for (unsigned y = 0; y < y_; ++y) host_walk(a_, g_, y);                      \
  })
#endif

// ---------------------------------------------------------------- the pieced dot of pk_cg.cpp and pk_minres.cpp
// The association of every dot of the two solvers, bit for bit the same on the device, on the host
// stand-in and in the emulators of tests/.  Index i belongs to piece i / 2048; thread t of the piece adds the terms at
// piece * 2048 + t + 256 j, j = 0 ... 7, in ascending j to 0.0 (an index beyond the length adds nothing) and leaves the sum in
// slot t of an LDS plane, one plane per simultaneous dot; the planes are reduced by the fixed tree of widths 128 ... 1
// (slot t += slot t + w) and thread q stores partial[q * n_pieces + piece].  The scalar step is one workgroup: per plane thread
// t adds the pieces t, t + 256, ... in ascending order to 0.0, the same tree follows, thread 0 decides.  No atomics, no
// dependence on the grid, the same bits from run to run.  The argument struct Args has partial, n_pieces and planes.
//
// The j = 0 ... 7 walk of a thread over its elements and the piece loop of a __global__ body stay in the units, written out per
// kernel: behind a callable or a shared template the compiler schedules pk_cg_init, pk_cg_update and pk_mr_update differently
// and flips a branch in pk_cg_dot -- equivalent code, but these kernels are held to byte-identical assembly (DESIGN.md
// section 20).  pk_merit.cpp's partial rows and its max columns are its own.
enum { PK_LIB_PER_THREAD = 8, PK_LIB_PIECE = PK_BLOCK * PK_LIB_PER_THREAD };
inline int64_t lib_dot_pieces(int64_t len) { return std::max<int64_t>(1, (len + PK_LIB_PIECE - 1) / PK_LIB_PIECE); }
// work items of a purely elementwise kernel: PK_BLOCK elements each
inline int64_t lib_elem_items(int64_t len) { return (len + PK_BLOCK - 1) / PK_BLOCK; }

// one step of the trees of `planes` dots, which share the barrier of the level: widths 128, 64 ... 1
PK_LIB_FN void lib_planes_step(double* s, int w, int t, int planes) {
  if (t >= w) return;
  for (int q = 0; q < planes; ++q) s[q * PK_BLOCK + t] = s[q * PK_BLOCK + t] + s[q * PK_BLOCK + t + w];
}

// thread q < planes behind the trees
template <class Args>
PK_LIB_FN void lib_store_partial(const Args& a, int64_t pc, int q, const double* s) {
  a.partial[(int64_t)q * a.n_pieces + pc] = s[q * PK_BLOCK];
}

// thread t of the scalar step: per plane the pieces t, t + 256, ... in ascending order
template <class Args>
PK_LIB_FN void lib_scalar_thread(const Args& a, int t, double* s) {
  for (int q = 0; q < a.planes; ++q) {
    double acc = 0.0;
    for (int64_t pc = t; pc < a.n_pieces; pc += PK_BLOCK) acc = acc + a.partial[(int64_t)q * a.n_pieces + pc];
    s[q * PK_BLOCK + t] = acc;
  }
}

#ifndef __HIPCC__
// the host stand-ins of the three kinds of kernel: pieces into `planes` of at most CAP planes (thread(pc, t, s) is the
// unit's), the scalar step (decide(a, s) is the unit's), PK_BLOCK elements per item (element(i) is the unit's)
template <int CAP, class Args, class Thread>
inline void lib_pieces_host(const Args& a, unsigned grid, int planes, Thread thread) {
  double s[CAP * PK_BLOCK];
  lib_walk_host(grid, a.n_pieces, [&](int64_t pc) {
    for (int t = 0; t < PK_BLOCK; ++t) thread(pc, t, s);
    lib_tree_host(lib_planes_step, s, planes);
    for (int q = 0; q < planes; ++q) lib_store_partial(a, pc, q, s);
  });
}
template <int CAP, class Args, class Decide>
inline void lib_scalar_host(const Args& a, Decide decide) {
  double s[CAP * PK_BLOCK];
  for (int t = 0; t < PK_BLOCK; ++t) lib_scalar_thread(a, t, s);
  lib_tree_host(lib_planes_step, s, (int)a.planes);
  decide(a, s);
}
template <class Element>
inline void lib_elements_host(unsigned grid, int64_t len, Element element) {
  lib_walk_host(grid, lib_elem_items(len), [&](int64_t item) {
    for (int64_t i = item * PK_BLOCK; i < std::min<int64_t>(len, (item + 1) * PK_BLOCK); ++i) element(i);
  });
}
#endif

#endif  // PK_LIBKERNEL_H
