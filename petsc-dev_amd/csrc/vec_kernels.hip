// Vec BLAS-1 kernels for gfx950.  All of them are HBM-bound streams of 16-byte (double2) loads / stores per lane.
// How the index space is dealt to workgroups decides the rate (profiles/r04_stream_probe*.log, n = 2^27 doubles per vector, beyond the
// 256 MiB Infinity Cache): a grid-stride loop over 2048 resident workgroups copies at 4.9 TB/s, ONE CONTIGUOUS TILE PER WORKGROUP
// ("flat": as many workgroups as tiles, the dispatcher hands out the next tile when a workgroup retires, so the tiles in flight
// form one compact window that slides through memory) at 6.0, with non-temporal accesses at 6.3-6.7; inside the cache (2^24) 7.7 ->
// 7.8-8.4 and the non-temporal hint costs 20 %.  So: element-wise kernels take one tile of 256 x 2 double2 per workgroup;
// reductions, whose workgroup count is also the number of partials the last workgroup has to add, keep <= 512 grid-striding
// workgroups for vectors that fit the cache (inside the cache the geometry makes no difference to a pure reader) and take contiguous
// runs of tiles of 256 x 4 double2, one run each for <= 4096 workgroups, for vectors of >= 256 MiB; those are also streamed
// non-temporally.  Compiled with -ffp-contract=off so a*x+y is a rounded multiply then a rounded add, as in the
// reference's C loops (src/vec/vec/impls/seq/{bvec1,bvec2,dvec2}.c).
#include "common.hpp"
#include <type_traits>

// Streaming accesses for operands nobody reads again soon.  In a CG iteration x and r are touched by the update sweep only and z
// by the AYPX that follows it only; loaded / stored non-temporally they stop evicting p, w and z from the L2 / Infinity Cache,
// which the neighbouring kernels re-read (measured on P7(256): fused update 0.183 -> 0.166 ms, whole iteration 0.414 -> 0.374 ms).
// The Jacobi diagonal, read once per iteration by the update alone, is a stream of the same kind (+3 % more); w, read here for the
// last time but still cached from the dot before, is better left alone.  Same values, same bits.
typedef double vk_v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 nt_load2(const double2 *p) {
  const vk_v2d t = __builtin_nontemporal_load(reinterpret_cast<const vk_v2d *>(p));
  double2 r; r.x = t.x; r.y = t.y; return r;
}
__device__ __forceinline__ void nt_store2(double2 *p, double2 v) {
  vk_v2d t; t.x = v.x; t.y = v.y;
  __builtin_nontemporal_store(t, reinterpret_cast<vk_v2d *>(p));
}
// Gram-Schmidt sweeps (VecMDot, VecMAXPY and their fused forms): when the nv basis vectors of a sweep are larger than the caches
// they are pure streams, and loaded non-temporally they leave the ONE vector the sweep shares with its neighbours (w: written by
// the product, read by MDot, read and written by MAXPY, scaled, gathered by the next product) in the L2 / Infinity Cache:
// GMRES(30)+Jacobi on P7(256) 1.045 -> 0.955 ms per iteration.  A basis that fits (P7(64): 16 x 2 MB) must stay cacheable:
// there the hint costs 20 %.  Threshold: half of the 256 MiB Infinity Cache.
static inline int gs_streams(size_t n, int nv) { return (size_t)nv * n * sizeof(double) > ((size_t)128 << 20); }

// ------------------------------------------------------------------------
// element-wise map:  out[i] = op(a[i], b[i], c[i])   (inputs may alias out)
// ------------------------------------------------------------------------
// big: vectors of >= 256 MiB cannot be cache-resident between two kernels: stream them (measured: +5-12 % there, -20 % inside the cache)
static inline int vec_streams(size_t n) { return n * sizeof(double) >= ((size_t)256 << 20); }
template <bool NT> __device__ __forceinline__ double2 ld2(const double2 *p) { return NT ? nt_load2(p) : *p; }
template <bool NT> __device__ __forceinline__ void st2(double2 *p, double2 v) { if (NT) nt_store2(p, v); else *p = v; }
// the same choice at run time (a functor member, uniform over the launch)
__device__ __forceinline__ double2 ldq(const double2 *p, int nt) { return nt ? nt_load2(p) : *p; }
__device__ __forceinline__ void stq(double2 *p, double2 v, int nt) { if (nt) nt_store2(p, v); else *p = v; }

// all of them 16-byte aligned (NULL, an operand a form of the kernel does not touch, counts as aligned)
template <class... P> static inline int all_aligned16(const P *...p) { return (mi355x_aligned16(p) && ...); }

// The element-wise tile walk.  vec_ok: workgroup b owns the tile [b * PER * 256, (b + 1) * PER * 256) of double2's and lane t its
// entries t, t + 256, .. : at2(i, U) is called once, for the U = PER double2's at i, i + 256, .. (U a std::integral_constant; at
// the edge of the vector, and for PER == 1, U = 1), so that a body can issue the loads of all its entries before the first store;
// lane 0 of workgroup 0 takes the odd last double with at1(n - 1).  An unaligned view: at1(k) over a scalar grid-stride loop.
template <int PER, class At2, class At1>
__device__ __forceinline__ void tile_walk(size_t n, int vec_ok, const At2 &at2, const At1 &at1) {
  const size_t tid = (size_t)blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (vec_ok) {
    const size_t n2 = n >> 1;
    const size_t i = (size_t)blockIdx.x * (PER * MI355X_BLOCK) + threadIdx.x;
    if (PER > 1 && i + (PER - 1) * MI355X_BLOCK < n2) at2(i, std::integral_constant<int, PER>());
    else if (i < n2) at2(i, std::integral_constant<int, 1>());
    if ((n & 1) && tid == 0) at1(n - 1);
  } else {
    const size_t stride = (size_t)gridDim.x * MI355X_BLOCK;
    for (size_t k = tid; k < n; k += stride) at1(k);
  }
}
// its workgroups: one per tile (an unaligned view: the capped grid of the scalar loop, 2 PER doubles per lane and trip)
template <int PER> static inline unsigned int tile_grid(size_t n, int vec_ok) {
  if (!vec_ok) return (unsigned int)mi355x_grid_for(n, 2 * PER);
  const size_t nt = ((n >> 1) + PER * MI355X_BLOCK - 1) / (PER * MI355X_BLOCK);
  return (unsigned int)(nt ? nt : 1);
}
// the U entries of a lane in its tile: v[u] <-> p[i + 256 u]
template <bool NT, int U> __device__ __forceinline__ void ld_tile(const double2 *p, size_t i, double2 (&v)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u) v[u] = ld2<NT>(p + i + u * MI355X_BLOCK);
}
template <bool NT, int U> __device__ __forceinline__ void st_tile(double2 *p, size_t i, const double2 (&v)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u) st2<NT>(p + i + u * MI355X_BLOCK, v[u]);
}
// A kernel over tiles of MI355X_MAP_TILE2 double2's comes in two instances, streamed (vec_streams) or not, and takes n and vec_ok last
template <class Kernel, class... A>
static int launch_tiles(mi355x_handle_t h, size_t n, int vec_ok, Kernel streamed, Kernel cached, A... args) {
  if (vec_streams(n)) hipLaunchKernelGGL(streamed, dim3(tile_grid<2>(n, vec_ok)), dim3(MI355X_BLOCK), 0, h->stream, args..., n, vec_ok);
  else hipLaunchKernelGGL(cached, dim3(tile_grid<2>(n, vec_ok)), dim3(MI355X_BLOCK), 0, h->stream, args..., n, vec_ok);
  MI355X_LAUNCH_CHECK();
  return 0;
}

template <int NIN, class Op, bool NT>
__global__ __launch_bounds__(MI355X_BLOCK) void map_kernel(Op op, const double *a, const double *b, const double *c,
                                                          double *out, size_t n, int vec_ok) {
  const double2 *a2 = reinterpret_cast<const double2 *>(a), *b2 = reinterpret_cast<const double2 *>(b);
  const double2 *c2 = reinterpret_cast<const double2 *>(c);
  double2 *o2 = reinterpret_cast<double2 *>(out);
  tile_walk<2>(n, vec_ok,
    [&](size_t i, auto u) {
      constexpr int U = decltype(u)::value;
      double2 av[U] = {}, bv[U] = {}, cv[U] = {}, r[U];
      if (NIN >= 1) ld_tile<NT>(a2, i, av);
      if (NIN >= 2) ld_tile<NT>(b2, i, bv);
      if (NIN >= 3) ld_tile<NT>(c2, i, cv);
#pragma unroll
      for (int j = 0; j < U; ++j) { r[j].x = op(av[j].x, bv[j].x, cv[j].x); r[j].y = op(av[j].y, bv[j].y, cv[j].y); }
      st_tile<NT>(o2, i, r);
    },
    [&](size_t k) { out[k] = op(NIN >= 1 ? a[k] : 0.0, NIN >= 2 ? b[k] : 0.0, NIN >= 3 ? c[k] : 0.0); });
}

template <int NIN, class Op>
static int launch_map(mi355x_handle_t h, Op op, const double *a, const double *b, const double *c, double *out, size_t n) {
  if (n == 0) return 0;
  return launch_tiles(h, n, all_aligned16(out, a, b, c), map_kernel<NIN, Op, true>, map_kernel<NIN, Op, false>, op, a, b, c, out);   // an input beyond NIN is NULL
}

struct OpSet      { double al; __device__ double operator()(double, double, double) const { return al; } };
struct OpCopy     { __device__ double operator()(double x, double, double) const { return x; } };
struct OpScale    { double al; __device__ double operator()(double x, double, double) const { return al * x; } };
struct OpAxpy     { double al; __device__ double operator()(double x, double y, double) const { return y + al * x; } };
struct OpAypx     { double al; __device__ double operator()(double x, double y, double) const { return x + al * y; } };
struct OpXmY      { __device__ double operator()(double x, double y, double) const { return x - y; } };
struct OpYmX      { __device__ double operator()(double x, double y, double) const { return y - x; } };
struct OpXpY      { __device__ double operator()(double x, double y, double) const { return y + x; } };
struct OpAxpby    { double al, be; __device__ double operator()(double x, double y, double) const { return al * x + be * y; } };
struct OpMul      { __device__ double operator()(double x, double y, double) const { return x * y; } };
struct OpDiv      { __device__ double operator()(double x, double y, double) const { return x / y; } };
struct OpRecip    { __device__ double operator()(double x, double, double) const { return x != 0.0 ? 1.0 / x : x; } };
struct OpJacInv   { __device__ double operator()(double x, double, double) const { return x == 0.0 ? 1.0 : 1.0 / x; } };
// z = al x + be y + ga z with the reference's four variants (bvec1.c:430-449)
struct OpAxpbypczA1 { double be, ga; __device__ double operator()(double x, double y, double z) const { return x + be * y + ga * z; } };
struct OpAxpbypczG1 { double al, be; __device__ double operator()(double x, double y, double z) const { return al * x + be * y + z; } };
struct OpAxpbypczG0 { double al, be; __device__ double operator()(double x, double y, double) const { return al * x + be * y; } };
struct OpAxpbypcz   { double al, be, ga; __device__ double operator()(double x, double y, double z) const { return al * x + be * y + ga * z; } };
struct OpShift    { double al; __device__ double operator()(double x, double, double) const { return x + al; } };
struct OpTriad    { double al; __device__ double operator()(double b, double c, double) const { return b + al * c; } };

// swap needs two outputs
__global__ __launch_bounds__(MI355X_BLOCK) void swap_kernel(double *x, double *y, size_t n) {
  const size_t stride = (size_t)gridDim.x * MI355X_BLOCK;
  for (size_t i = (size_t)blockIdx.x * MI355X_BLOCK + threadIdx.x; i < n; i += stride) {
    double t = x[i];
    x[i] = y[i];
    y[i] = t;
  }
}

// ------------------------------------------------------------------------
// MAXPY: x += (a0 y0 + .. ) [group 0, G0 vectors] ; x += (..) [group 1, G1 vectors]
// groups and left-to-right sums as petscaxpy.h:101-110 / dvec2.c:853-900
// ------------------------------------------------------------------------
struct MaxpyArgs {
  const double *y[32];
  double a[32];
  int nt;
};

template <int G>
__device__ __forceinline__ double group_sum(const double *a, const double *v) {
  double s = a[0] * v[0];
#pragma unroll
  for (int j = 1; j < G; ++j) s = s + a[j] * v[j];
  return s;
}

// x += group 0 (G0 = 1..4 vectors), then NG4 groups of four, each group summed left to right and added to x in turn:
// the association of petscaxpy.h:101-110.  Up to 32 vectors per sweep, so x is read and written once per 32
// (GMRES(30)'s largest update in one sweep: 0.79 ms instead of 0.86 ms at n = 2^24).
template <int G0, int NG4>
__device__ __forceinline__ double maxpy_elem(double xv, const double *a, const double *v) {
  xv = xv + group_sum<G0>(a, v);
#pragma unroll
  for (int g = 0; g < NG4; ++g) xv = xv + group_sum<4>(a + G0 + 4 * g, v + G0 + 4 * g);
  return xv;
}

// the double2's at i of the NV basis vectors, streamed past the caches or not (see gs_streams())
template <int NV>
__device__ __forceinline__ void load_basis(const double *const *y, size_t i, int nt, double2 (&yv)[NV]) {
  if (nt) {
#pragma unroll
    for (int j = 0; j < NV; ++j) yv[j] = nt_load2(reinterpret_cast<const double2 *>(y[j]) + i);
  } else {
#pragma unroll
    for (int j = 0; j < NV; ++j) yv[j] = reinterpret_cast<const double2 *>(y[j])[i];
  }
}
// x after the grouped update: the double2 at i (the basis is requested first, then x) and the double at k
template <int G0, int NG4>
__device__ __forceinline__ double2 maxpy_at2(const double *const *y, const double *a, int nt, const double *x, size_t i) {
  constexpr int NV = G0 + 4 * NG4;
  double2 yv[NV];
  load_basis<NV>(y, i, nt, yv);
  double2 xv = reinterpret_cast<const double2 *>(x)[i];
  double lo[NV], hi[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) { lo[j] = yv[j].x; hi[j] = yv[j].y; }
  xv.x = maxpy_elem<G0, NG4>(xv.x, a, lo);
  xv.y = maxpy_elem<G0, NG4>(xv.y, a, hi);
  return xv;
}
template <int G0, int NG4>
__device__ __forceinline__ double maxpy_at1(const double *const *y, const double *a, const double *x, size_t k) {
  constexpr int NV = G0 + 4 * NG4;
  double v[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = y[j][k];
  return maxpy_elem<G0, NG4>(x[k], a, v);
}

// one double2 of every stream per lane, one contiguous tile of 256 per workgroup
template <int G0, int NG4>
__global__ __launch_bounds__(MI355X_BLOCK) void maxpy_kernel(MaxpyArgs args, double *x, size_t n, int vec_ok) {
  tile_walk<1>(n, vec_ok,
    [&](size_t i, auto) { reinterpret_cast<double2 *>(x)[i] = maxpy_at2<G0, NG4>(args.y, args.a, args.nt, x, i); },
    [&](size_t k) { x[k] = maxpy_at1<G0, NG4>(args.y, args.a, x, k); });
}

// VecMAXPY's chunking of nv vectors into sweeps: f(pos, g0, ng4) for the vectors from pos on.  First group: the remainder
// nv % 4 if there is one (dvec2.c:853-877 handles it first), else four; then up to seven more groups of four in the same sweep.
template <class F> static int for_each_sweep(int nv, F f) {
  const int rem = nv & 3;
  for (int pos = 0; pos < nv;) {
    const int g0 = (pos == 0 && rem) ? rem : 4;
    int ng4 = (nv - pos - g0) / 4;
    if (ng4 > 7) ng4 = 7;
    const int rc = f(pos, g0, ng4);
    if (rc) return rc;
    pos += g0 + 4 * ng4;
  }
  return 0;
}
// ... and from (g0, ng4) to the template instance: f(G0, NG4) with both a std::integral_constant
template <class F> static int with_groups(int g0, int ng4, F f) {
#define GS_CASE(G, N4) case (G) * 10 + (N4): return f(std::integral_constant<int, G>(), std::integral_constant<int, N4>())
#define GS_ROW(G) GS_CASE(G, 0); GS_CASE(G, 1); GS_CASE(G, 2); GS_CASE(G, 3); GS_CASE(G, 4); GS_CASE(G, 5); GS_CASE(G, 6); GS_CASE(G, 7)
  switch (g0 * 10 + ng4) {
    GS_ROW(1); GS_ROW(2); GS_ROW(3); GS_ROW(4);
    default: return (int)hipErrorInvalidValue;
  }
#undef GS_ROW
#undef GS_CASE
}
// dst[j] = y[j] for the cnt vectors of a sweep; returns whether all of them are 16-byte aligned
static inline int fill_basis(const double **dst, const double *const *y, int cnt) {
  int ok = 1;
  for (int j = 0; j < cnt; ++j) { dst[j] = y[j]; ok = ok && mi355x_aligned16(y[j]); }
  return ok;
}

// ------------------------------------------------------------------------
// reductions: single launch, fixed tree, last-arriving workgroup finishes
// ------------------------------------------------------------------------
enum { RED_SUM = 0, RED_MAX = 1, RED_ARGMAX = 2, RED_ARGMIN = 3 };
// RED_ARGMAX / RED_ARGMIN (NOUT == 2): acc is ONE (value, location) pair, the location a double (exact below 2^53, the way VecMax_MPI
// carries it; < 0: no element met yet).  VecMax_Seq / VecMin_Seq (dvec2.c) start from x[0] and replace on a strict > / <: of the
// elements that are no NaN the extremum with the lowest index, carrying that element's own value (-0.0 and +0.0 tie).  As a rule for
// combining pairs: a NaN and an empty pair are never taken, a larger value is, an equal value only with a lower index.  Locations
// are distinct, so the rule orders the pairs totally and the tree may combine them in any order.  (x[0] being NaN: ExtremumF::epilogue.)
template <int MODE> struct is_pair_mode { static constexpr bool value = (MODE == RED_ARGMAX || MODE == RED_ARGMIN); };
template <int MODE>
__device__ __forceinline__ void pair_take(double (&a)[2], double v, double idx) {
  if (idx < 0.0 || v != v) return;
  const bool better = a[1] < 0.0 || (MODE == RED_ARGMAX ? v > a[0] : v < a[0]) || (v == a[0] && idx < a[1]);
  if (better) { a[0] = v; a[1] = idx; }
}
template <int MODE>
__device__ __forceinline__ void wave_pair(double (&a)[2]) {
#pragma unroll
  for (int off = MI355X_WAVE / 2; off > 0; off >>= 1) {
    const double v = __shfl_down(a[0], off, MI355X_WAVE), idx = __shfl_down(a[1], off, MI355X_WAVE);
    pair_take<MODE>(a, v, idx);
  }
}

template <int NOUT, int MODE, bool PUBLISH = false>
__device__ __forceinline__ void block_reduce_store(double (&acc)[NOUT], double *dst /* NOUT doubles */, double (*lds)[NOUT]) {
  const int lane = threadIdx.x & (MI355X_WAVE - 1);
  const int wave = threadIdx.x / MI355X_WAVE;
  if constexpr (is_pair_mode<MODE>::value) {
    static_assert(NOUT == 2, "a pair reduction carries (value, location)");
    wave_pair<MODE>(acc);
    if (lane == 0) { lds[wave][0] = acc[0]; lds[wave][1] = acc[1]; }
    __syncthreads();
    if (threadIdx.x == 0) {
      double s[2] = {lds[0][0], lds[0][1]};
#pragma unroll
      for (int w = 1; w < MI355X_BLOCK / MI355X_WAVE; ++w) pair_take<MODE>(s, lds[w][0], lds[w][1]);
      if (PUBLISH) {
        __hip_atomic_store(dst, s[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(dst + 1, s[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else { dst[0] = s[0]; dst[1] = s[1]; }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NOUT; ++j) {
    double v = (MODE == RED_MAX) ? wave_max(acc[j]) : wave_sum(acc[j]);
    if (lane == 0) lds[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < NOUT) {
    double s = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < MI355X_BLOCK / MI355X_WAVE; ++w)
      s = (MODE == RED_MAX) ? nanmax(s, lds[w][threadIdx.x]) : s + lds[w][threadIdx.x];
    // a partial that another workgroup will read is stored write-through (sc1): it reaches the memory side
    // without an L2 write-back fence per workgroup
    if (PUBLISH) __hip_atomic_store(dst + threadIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else dst[threadIdx.x] = s;
  }
}

// After the result has been stored: make it visible to the host, then store the completion number the host polls.
__device__ __forceinline__ void publish_to_host(unsigned long long *host_seq, unsigned long long seq) {
  __syncthreads();                       // the result stores of lanes < NOUT are done
  if (host_seq && threadIdx.x == 0) {
    __threadfence_system();
    __hip_atomic_store(host_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// KSPSolve_CG's step length a = beta / dpi with dpi = p'w still in device memory, and the reference's break-down tests on dpi
// (cg.c:196-199).  When one fires a = 0 and nothing may be modified; the host, which receives dpi with the sums, takes the exit.
struct CGStepLen {
  double beta, dpiold;
  int check_sign;
  const double *dpi_ptr;
  __device__ __forceinline__ bool operator()(double &a) const {
    const double dpi = *dpi_ptr;
    const bool bad = !(dpi == dpi) || fabs(dpi) == __builtin_huge_val() || dpi == 0.0 || (check_sign && dpi * dpiold <= 0.0);
    a = bad ? 0.0 : beta / dpi;
    return !bad;
  }
};

// y = x + (num/den) y with the scalar's numerator still in device memory (KSPSolve_CG: b = beta_new/beta_old, beta_new
// being the z'r the previous kernel on the stream has just reduced).  VecAYPX_Seq's special case alpha == 0 -> copy
// (dvec2.c:980) is kept; alpha == +-1 need no special form (x + 1*y and x + (-1)*y are the bits of x + y and x - y).
// WX: the same pass also does KSPSolve_CG's sol += a y (cg.c:206) with the y it is about to overwrite, so the update sweep
// before it (CGUpdateDevF with x == NULL) reads neither p nor x: 12 vector passes per CG iteration instead of 13.  a is
// formed as the update forms it (CGStepLen); for a == 0 (a refused step) sol is left alone, as VecAXPY leaves y alone
// (bvec1.c:253).  x (= z) and sol have their last reader of the iteration here: streamed (see nt_load2).
template <bool NT, bool WX>
__global__ __launch_bounds__(MI355X_BLOCK) void aypx_dev_kernel(const double *num, double den, const double *x, double *y, CGStepLen sl, double *sol,
                                                              size_t n, int vec_ok) {
  const double alpha = *num / den;
  const bool copy = (alpha == 0.0);
  double a = 0.0;
  if (WX) sl(a);
  const bool ax = WX && a != 0.0;
  const auto y_new = [=](double xv, double yv) { return copy ? xv : xv + alpha * yv; };
  const double2 *x2 = reinterpret_cast<const double2 *>(x);
  double2 *y2 = reinterpret_cast<double2 *>(y), *s2 = reinterpret_cast<double2 *>(sol);
  tile_walk<2>(n, vec_ok,
    [&](size_t i, auto u) {
      constexpr int U = decltype(u)::value;
      double2 xv[U], yv[U], r[U];
      ld_tile<true>(x2, i, xv);                    // x = z: its last reader (see nt_load2)
      ld_tile<NT>(y2, i, yv);
      if (ax) {
        double2 sv[U];
        ld_tile<true>(s2, i, sv);
#pragma unroll
        for (int j = 0; j < U; ++j) { sv[j].x = sv[j].x + a * yv[j].x; sv[j].y = sv[j].y + a * yv[j].y; }
        st_tile<true>(s2, i, sv);
      }
#pragma unroll
      for (int j = 0; j < U; ++j) { r[j].x = y_new(xv[j].x, yv[j].x); r[j].y = y_new(xv[j].y, yv[j].y); }
      st_tile<NT>(y2, i, r);
    },
    [&](size_t k) {
      if (ax) sol[k] = sol[k] + a * y[k];
      y[k] = y_new(x[k], y[k]);
    });
}

// x += *num / den with the numerator still in device memory (MatNullSpaceRemove's constant part, matnull.c: the VecSum the kernel
// before this one on the stream has just reduced, over -N): the quotient is formed once per lane, IEEE division as on the host
template <bool NT>
__global__ __launch_bounds__(MI355X_BLOCK) void shift_dev_kernel(const double *num, double den, double *x, size_t n, int vec_ok) {
  const double alpha = *num / den;
  double2 *x2 = reinterpret_cast<double2 *>(x);
  tile_walk<2>(n, vec_ok,
    [&](size_t i, auto u) {
      double2 v[decltype(u)::value];
      ld_tile<NT>(x2, i, v);
      for (double2 &e : v) { e.x = e.x + alpha; e.y = e.y + alpha; }
      st_tile<NT>(x2, i, v);
    },
    [&](size_t k) { x[k] = x[k] + alpha; });
}

// copy <= 64 doubles from device memory to the handle's pinned scratch, then store the completion number the host
// polls (mi355x_handle_wait_result): how a result that had to stay on the device first (RCCL all-reduce, a later kernel
// reading it) reaches the host without a stream synchronisation
__global__ void publish_kernel(const double *src, double *host_dst, int count, unsigned long long *host_seq, unsigned long long seq) {
  if ((int)threadIdx.x < count) host_dst[threadIdx.x] = src[threadIdx.x];
  publish_to_host(host_seq, seq);
}

template <int NOUT> __device__ __forceinline__ void zero(double (&acc)[NOUT]) {
#pragma unroll
  for (int j = 0; j < NOUT; ++j) acc[j] = 0.0;
}
// what a lane starts from: zeros; the pair modes: no element met yet
template <int MODE, int NOUT> __device__ __forceinline__ void init_acc(double (&acc)[NOUT]) {
  zero(acc);
  if (is_pair_mode<MODE>::value) acc[NOUT - 1] = -1.0;
}

// The hand-off of a launch of several workgroups: each stores its partial sums; the one that arrives last gets true and, in acc,
// every lane's share of all partials.
template <int NOUT, int MODE>
__device__ __forceinline__ bool last_workgroup_gathers(double (&acc)[NOUT], double *partials, unsigned int *ticket, double (*lds)[NOUT]) {
  __shared__ int is_last;
  block_reduce_store<NOUT, MODE, true>(acc, partials + (size_t)blockIdx.x * NOUT, lds);
  // Publish: the partials were stored write-through (sc1) by lanes of wavefront 0; once those stores have left
  // (vmcnt(0)) lane 0 of the SAME wavefront takes a ticket with a relaxed agent-scope add.  The workgroup that draws
  // the last ticket acquires (invalidates its CU's L1) and reads every partial with sc1 loads.  This is the
  // write-through form of the hand-off MI355X_MICROARCH.md lists as valid on gfx950 ("sc1 slab stores need no release
  // fence -> every storing wave s_waitcnt vmcnt(0) -> one lane's relaxed agent fetch_add; the reducer acquires");
  // it is a property of this ISA, not of the HIP memory model.  -DMI355X_REDUCE_RELEASE=1 builds the model-conformant
  // form (agent-scope release fence before the ticket: an L2 write-back per workgroup, dot 0.044 -> 0.106 ms at n = 2^24).
  if (threadIdx.x < MI355X_WAVE) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (threadIdx.x == 0) {
#if defined(MI355X_REDUCE_RELEASE) && MI355X_REDUCE_RELEASE
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
      unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int last = (t == gridDim.x - 1);
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      is_last = last;
    }
  }
  __syncthreads();
  if (!is_last) return false;
  // last-arriving workgroup: sum the per-workgroup partials in workgroup order (pairs: combine them, see pair_take)
  init_acc<MODE>(acc);
  // (a lane's partials b = t, t + 256, ... are added in that order; up to four workgroups' worth requested together)
  for (unsigned int b0 = threadIdx.x; b0 < gridDim.x; b0 += 4 * MI355X_BLOCK) {
    double v[4][NOUT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned int b = b0 + u * MI355X_BLOCK;
#pragma unroll
      for (int j = 0; j < NOUT; ++j) v[u][j] = __hip_atomic_load(partials + (size_t)(b < gridDim.x ? b : b0) * NOUT + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (b0 + u * MI355X_BLOCK < gridDim.x) {
        if constexpr (is_pair_mode<MODE>::value) pair_take<MODE>(acc, v[u][0], v[u][1]);
        else {
#pragma unroll
          for (int j = 0; j < NOUT; ++j) acc[j] = (MODE == RED_MAX) ? nanmax(acc[j], v[u][j]) : acc[j] + v[u][j];
        }
      }
    }
  }
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every workgroup has drawn its ticket
  __syncthreads();
  return true;
}

// functors that need a once-per-lane hook before the sweep specialise this
template <class F> struct has_prologue { static constexpr bool value = false; };
// ... a hook on the finished result (the lane that stored it: lane 0) specialise this
template <class F> struct has_epilogue { static constexpr bool value = false; };

// F::accum(i2 or i, acc): adds element contributions
// RUNS == false: grid-stride (lane t of workgroup b meets double2's b * 256 + t, + grid * 256, ...): vectors that live in the caches.
// RUNS == true: workgroup b owns a contiguous run of tiles of MI355X_TILE2 double2's, [s0, s1), and lane t meets s0 + t, s0 + t + 256,
// ...: vectors of >= 256 MiB, where one compact window of tiles in flight streams 6.0-7.0 TB/s and 512 strided workgroups 4.9-6.1
// (profiles/r04_stream_probe*.log).  The functors' sweeps take a first index, a step and an end, so they serve both.  The oracle's
// device-order emulation (oracle/vecmat_oracle.c dev_reduce) restates both geometries and the size that separates them: change together.
template <int NOUT, int MODE, class F, bool RUNS>
__global__ __launch_bounds__(MI355X_BLOCK) void reduce_kernel(F f, size_t n, int vec_ok, double *partials,
                                                             unsigned int *ticket, double *out, double *host_copy,
                                                             unsigned long long *host_seq, unsigned long long seq) {
  __shared__ double lds[MI355X_BLOCK / MI355X_WAVE][NOUT];
  const size_t tid = (size_t)blockIdx.x * MI355X_BLOCK + threadIdx.x;
  double acc[NOUT];
  init_acc<MODE>(acc);
  if constexpr (has_prologue<F>::value) f.prologue(tid, acc);
  if (vec_ok) {
    const size_t n2 = n >> 1;
    if (RUNS) {
      const size_t ntiles = (n2 + MI355X_TILE2 - 1) / MI355X_TILE2;
      const size_t per = (ntiles + gridDim.x - 1) / gridDim.x;
      size_t s0 = (size_t)blockIdx.x * per * MI355X_TILE2, s1 = s0 + per * MI355X_TILE2;
      if (s0 > n2) s0 = n2;
      if (s1 > n2) s1 = n2;
      f.template sweep<NOUT>(s0 + threadIdx.x, (size_t)MI355X_BLOCK, s1, acc);
    } else {
      f.template sweep<NOUT>(tid, (size_t)gridDim.x * MI355X_BLOCK, n2, acc);
    }
    if ((n & 1) && tid == 0) f.accum1(n - 1, acc);
  } else {
    const size_t stride = (size_t)gridDim.x * MI355X_BLOCK;
    for (size_t i = tid; i < n; i += stride) f.accum1(i, acc);
  }
  if (gridDim.x > 1 && !last_workgroup_gathers<NOUT, MODE>(acc, partials, ticket, lds)) return;   // a single workgroup needs no hand-off
  block_reduce_store<NOUT, MODE>(acc, out, lds);
  if constexpr (has_epilogue<F>::value) { if (threadIdx.x == 0) f.epilogue(n, out); }
  // a result that stays on the device for the next kernel can be handed to the host as well (same lanes that stored it)
  if (host_copy) { __syncthreads(); if (threadIdx.x < NOUT) host_copy[threadIdx.x] = out[threadIdx.x]; }
  publish_to_host(host_seq, seq);
}

template <int NOUT, int MODE, class F>
static int launch_reduce(mi355x_handle_t h, F f, size_t n, int vec_ok, double *out, bool also_to_host = false) {
  // vectors that fit the caches: at most 512 workgroups, 2 per CU (measured on the CG iteration at n = 2^24, one box, same process
  // order: 256 -> 0.541 ms, 384 -> 0.535, 512 -> 0.523, 768 -> 0.529, 1024 -> 0.534, 2048 -> 0.536; 8192 with one tile each: 0.56),
  // grid-stride; the last one sums <= 512 partials.  Vectors of >= 256 MiB: contiguous runs of tiles for <= 4096 workgroups.  The
  // oracle's device-order emulation (oracle/vecmat_oracle.c dev_reduce) restates both: change together.
  const bool runs = vec_streams(n) != 0;
  int grid;
  if (runs) {
    const size_t ntiles = ((n >> 1) + MI355X_TILE2 - 1) / MI355X_TILE2;
    grid = (int)(ntiles > MI355X_REDUCE_GRID_CAP_BIG ? MI355X_REDUCE_GRID_CAP_BIG : ntiles);
  } else {
    grid = mi355x_grid_for(n, 16);
    if (grid > MI355X_REDUCE_GRID_CAP) grid = MI355X_REDUCE_GRID_CAP;
  }
  // a result that goes to the handle's pinned scratch is followed by a completion number (mi355x_handle_wait_result)
  unsigned long long *hs = nullptr, seq = 0;
  double *host_copy = nullptr;
  if (out >= h->host_scratch && out < h->host_scratch + MI355X_SCRATCH_DOUBLES) {
    hs = const_cast<unsigned long long *>(h->host_seq);
    seq = ++h->seq;
  } else if (also_to_host) {   // result to `out` (device) AND to the first NOUT pinned slots, then the completion number
    hs = const_cast<unsigned long long *>(h->host_seq);
    seq = ++h->seq;
    host_copy = h->host_scratch;
  }
  if (runs) hipLaunchKernelGGL((reduce_kernel<NOUT, MODE, F, true>), dim3(grid), dim3(MI355X_BLOCK), 0, h->stream, f, n, vec_ok,
                               h->partials, h->ticket, out, host_copy, hs, seq);
  else hipLaunchKernelGGL((reduce_kernel<NOUT, MODE, F, false>), dim3(grid), dim3(MI355X_BLOCK), 0, h->stream, f, n, vec_ok,
                          h->partials, h->ticket, out, host_copy, hs, seq);
  MI355X_LAUNCH_CHECK();
  return 0;
}

// default sweep: four grid-stride iterations at a time (i, i + stride, i + 2 stride, i + 3 stride in that order, .x then .y within
// each), then one at a time.  BATCHED_SWEEP: the functor has a form of the four, accum2x4, that issues all their loads together.
#define SWEEP_BY_FOUR(FOUR)                                                                          \
  template <int NOUT_>                                                                               \
  __device__ __forceinline__ void sweep(size_t tid, size_t stride, size_t n2, double (&a)[NOUT_]) const { \
    size_t i = tid;                                                                                  \
    for (; i + 3 * stride < n2; i += 4 * stride) { FOUR; }                                           \
    for (; i < n2; i += stride) accum2(i, a);                                                        \
  }
#define DEFAULT_SWEEP() SWEEP_BY_FOUR(accum2(i, a); accum2(i + stride, a); accum2(i + 2 * stride, a); accum2(i + 3 * stride, a))
#define BATCHED_SWEEP() SWEEP_BY_FOUR(accum2x4(i, stride, a))

struct DotF {
  const double *x, *y;
  int nt = 0;                  // vectors too large for the cache: streamed (vec_streams)
  BATCHED_SWEEP()
  __device__ void accum2x4(size_t i, size_t st, double (&a)[1]) const {
    const double2 *x2 = reinterpret_cast<const double2 *>(x), *y2 = reinterpret_cast<const double2 *>(y);
    double2 xv0 = ldq(x2 + i, nt), xv1 = ldq(x2 + i + st, nt), xv2 = ldq(x2 + i + 2 * st, nt), xv3 = ldq(x2 + i + 3 * st, nt);
    double2 yv0 = ldq(y2 + i, nt), yv1 = ldq(y2 + i + st, nt), yv2 = ldq(y2 + i + 2 * st, nt), yv3 = ldq(y2 + i + 3 * st, nt);
    a[0] += xv0.x * yv0.x; a[0] += xv0.y * yv0.y; a[0] += xv1.x * yv1.x; a[0] += xv1.y * yv1.y;
    a[0] += xv2.x * yv2.x; a[0] += xv2.y * yv2.y; a[0] += xv3.x * yv3.x; a[0] += xv3.y * yv3.y;
  }
  __device__ void accum1(size_t i, double (&a)[1]) const { a[0] += x[i] * y[i]; }
  __device__ void accum2(size_t i, double (&a)[1]) const {
    double2 xv = reinterpret_cast<const double2 *>(x)[i], yv = reinterpret_cast<const double2 *>(y)[i];
    a[0] += xv.x * yv.x;
    a[0] += xv.y * yv.y;
  }
};
// VecSum: DotF with y == 1.0 everywhere (x * 1.0 is x): same lanes, same order, same streaming threshold -- the bits of
// mi355x_vec_dot(x, ones)
struct SumF {
  const double *x;
  int nt = 0;
  BATCHED_SWEEP()
  __device__ void accum2x4(size_t i, size_t st, double (&a)[1]) const {
    const double2 *x2 = reinterpret_cast<const double2 *>(x);
    double2 v0 = ldq(x2 + i, nt), v1 = ldq(x2 + i + st, nt), v2 = ldq(x2 + i + 2 * st, nt), v3 = ldq(x2 + i + 3 * st, nt);
    a[0] += v0.x; a[0] += v0.y; a[0] += v1.x; a[0] += v1.y;
    a[0] += v2.x; a[0] += v2.y; a[0] += v3.x; a[0] += v3.y;
  }
  __device__ void accum1(size_t i, double (&a)[1]) const { a[0] += x[i]; }
  __device__ void accum2(size_t i, double (&a)[1]) const {
    double2 xv = reinterpret_cast<const double2 *>(x)[i];
    a[0] += xv.x;
    a[0] += xv.y;
  }
};
// VecMax_Seq / VecMin_Seq (dvec2.c): the (value, location) pair under launch_reduce<2, RED_ARGMAX / RED_ARGMIN>.  The combining rule
// never takes a NaN; the reference starts from x[0] and nothing compares greater (or less) than a NaN, so a NaN at position 0 IS the
// answer: the epilogue puts it there.  No element at all: PETSC_MIN_REAL / PETSC_MAX_REAL and location -1.
template <int MODE>
struct ExtremumF {
  const double *x;
  DEFAULT_SWEEP()
  __device__ void accum1(size_t i, double (&a)[2]) const { pair_take<MODE>(a, x[i], (double)i); }
  __device__ void accum2(size_t i, double (&a)[2]) const {
    double2 xv = reinterpret_cast<const double2 *>(x)[i];
    pair_take<MODE>(a, xv.x, (double)(2 * i));
    pair_take<MODE>(a, xv.y, (double)(2 * i + 1));
  }
  __device__ void epilogue(size_t n, double *out) const {
    if (n == 0) { out[0] = MODE == RED_ARGMAX ? -1.7976931348623157e308 : 1.7976931348623157e308; out[1] = -1.0; }
    else if (x[0] != x[0]) { out[0] = x[0]; out[1] = 0.0; }
  }
};
template <int MODE> struct has_epilogue<ExtremumF<MODE>> { static constexpr bool value = true; };
struct SumSqF {
  const double *x;
  int nt = 0;
  BATCHED_SWEEP()
  __device__ void accum2x4(size_t i, size_t st, double (&a)[1]) const {
    const double2 *x2 = reinterpret_cast<const double2 *>(x);
    double2 v0 = ldq(x2 + i, nt), v1 = ldq(x2 + i + st, nt), v2 = ldq(x2 + i + 2 * st, nt), v3 = ldq(x2 + i + 3 * st, nt);
    a[0] += v0.x * v0.x; a[0] += v0.y * v0.y; a[0] += v1.x * v1.x; a[0] += v1.y * v1.y;
    a[0] += v2.x * v2.x; a[0] += v2.y * v2.y; a[0] += v3.x * v3.x; a[0] += v3.y * v3.y;
  }
  __device__ void accum1(size_t i, double (&a)[1]) const { a[0] += x[i] * x[i]; }
  __device__ void accum2(size_t i, double (&a)[1]) const {
    double2 xv = reinterpret_cast<const double2 *>(x)[i];
    a[0] += xv.x * xv.x;
    a[0] += xv.y * xv.y;
  }
};
struct SumAbsF {
  const double *x;
  DEFAULT_SWEEP()
  __device__ void accum1(size_t i, double (&a)[1]) const { a[0] += fabs(x[i]); }
  __device__ void accum2(size_t i, double (&a)[1]) const {
    double2 xv = reinterpret_cast<const double2 *>(x)[i];
    a[0] += fabs(xv.x);
    a[0] += fabs(xv.y);
  }
};
struct MaxAbsF {
  const double *x;
  DEFAULT_SWEEP()
  __device__ void accum1(size_t i, double (&a)[1]) const { a[0] = nanmax(a[0], fabs(x[i])); }
  __device__ void accum2(size_t i, double (&a)[1]) const {
    double2 xv = reinterpret_cast<const double2 *>(x)[i];
    a[0] = nanmax(a[0], fabs(xv.x));
    a[0] = nanmax(a[0], fabs(xv.y));
  }
};
struct Norm12F {
  const double *x;
  DEFAULT_SWEEP()
  __device__ void accum1(size_t i, double (&a)[2]) const { a[0] += fabs(x[i]); a[1] += x[i] * x[i]; }
  __device__ void accum2(size_t i, double (&a)[2]) const {
    double2 xv = reinterpret_cast<const double2 *>(x)[i];
    a[0] += fabs(xv.x); a[1] += xv.x * xv.x;
    a[0] += fabs(xv.y); a[1] += xv.y * xv.y;
  }
};
struct DotNorm2F {
  const double *s, *t;
  DEFAULT_SWEEP()
  __device__ void accum1(size_t i, double (&a)[2]) const { a[0] += s[i] * t[i]; a[1] += t[i] * t[i]; }
  __device__ void accum2(size_t i, double (&a)[2]) const {
    double2 sv = reinterpret_cast<const double2 *>(s)[i], tv = reinterpret_cast<const double2 *>(t)[i];
    a[0] += sv.x * tv.x; a[1] += tv.x * tv.x;
    a[0] += sv.y * tv.y; a[1] += tv.y * tv.y;
  }
};
// One CG update sweep (KSPSolve_CG cg.c:206-232 with PCApply_Jacobi jacobi.c:266-277 in between):
//   x += a p ; r += (-a) w ; z = r .* d ; out = { sum z*z , sum z*r , sum r*r }
// Element-wise arithmetic is that of the separate kernels (OpAxpy, OpAxpy, OpMul) and each lane meets its elements in
// the same order as SumSqF / DotF do under launch_reduce, so x, r, z and both sums carry the same bits as the five
// separate launches; HBM passes drop from 12 to 8.
// WX == false: x += a p is left to the AYPX that follows (aypx_dev_kernel<NT, true>), and neither p nor x is read here:
// 5 vector passes instead of 8; same lanes, same order, same sums.
struct CGVecs {
  const double *p, *w, *d;
  double *x, *r, *z;
  int big;                     // vectors too large for the cache: p, w and z are streams as well (vec_streams)
};
template <bool WX, int NOUT>
__device__ __forceinline__ void cg_step(double a, double pv, double wv, double dv, double &xv, double &rv, double &zv, double (&acc)[NOUT]) {
  if (a != 0.0) {              // VecAXPY leaves y alone for alpha == 0 (bvec1.c:253); uniform over the launch
    if (WX) xv = xv + a * pv;
    rv = rv + (-a) * wv;
  }
  zv = rv * dv;
  acc[0] += zv * zv;
  acc[1] += zv * rv;
  acc[2] += rv * rv;           // VecNorm(R) for KSP_NORM_UNPRECONDITIONED (cg.c:246)
}
template <bool WX, int NOUT>
__device__ __forceinline__ void cg_sweep(const CGVecs &v, double a, size_t tid, size_t stride, size_t n2, double (&acc)[NOUT]) {
  const double2 *p2 = reinterpret_cast<const double2 *>(v.p), *w2 = reinterpret_cast<const double2 *>(v.w);
  const double2 *d2 = reinterpret_cast<const double2 *>(v.d);
  const double2 one2 = {1.0, 1.0}, zero2 = {0.0, 0.0};
  double2 *x2 = reinterpret_cast<double2 *>(v.x), *r2 = reinterpret_cast<double2 *>(v.r), *z2 = reinterpret_cast<double2 *>(v.z);
  const int big = v.big;
  size_t i = tid;
  for (; i + stride < n2; i += 2 * stride) {
    double2 pv0 = WX ? ldq(p2 + i, big) : zero2, pv1 = WX ? ldq(p2 + i + stride, big) : zero2, wv0 = ldq(w2 + i, big), wv1 = ldq(w2 + i + stride, big), dv0 = d2 ? nt_load2(d2 + i) : one2, dv1 = d2 ? nt_load2(d2 + i + stride) : one2;
    double2 xv0 = WX ? nt_load2(x2 + i) : zero2, xv1 = WX ? nt_load2(x2 + i + stride) : zero2, rv0 = nt_load2(r2 + i), rv1 = nt_load2(r2 + i + stride), zv0, zv1;
    cg_step<WX>(a, pv0.x, wv0.x, dv0.x, xv0.x, rv0.x, zv0.x, acc); cg_step<WX>(a, pv0.y, wv0.y, dv0.y, xv0.y, rv0.y, zv0.y, acc);
    cg_step<WX>(a, pv1.x, wv1.x, dv1.x, xv1.x, rv1.x, zv1.x, acc); cg_step<WX>(a, pv1.y, wv1.y, dv1.y, xv1.y, rv1.y, zv1.y, acc);
    if (WX) nt_store2(x2 + i, xv0);
    nt_store2(r2 + i, rv0); stq(z2 + i, zv0, big);
    if (WX) nt_store2(x2 + i + stride, xv1);
    nt_store2(r2 + i + stride, rv1); stq(z2 + i + stride, zv1, big);
  }
  for (; i < n2; i += stride) {
    double2 pv = WX ? p2[i] : zero2, wv = w2[i], dv = d2 ? nt_load2(d2 + i) : one2, xv = WX ? nt_load2(x2 + i) : zero2, rv = nt_load2(r2 + i), zv;
    cg_step<WX>(a, pv.x, wv.x, dv.x, xv.x, rv.x, zv.x, acc); cg_step<WX>(a, pv.y, wv.y, dv.y, xv.y, rv.y, zv.y, acc);
    if (WX) nt_store2(x2 + i, xv);
    nt_store2(r2 + i, rv); z2[i] = zv;
  }
}
template <bool WX, int NOUT>
__device__ __forceinline__ void cg_accum1(const CGVecs &v, double a, size_t i, double (&acc)[NOUT]) {
  double xv = WX ? v.x[i] : 0.0, rv = v.r[i], zv;
  cg_step<WX>(a, WX ? v.p[i] : 0.0, v.w[i], v.d ? v.d[i] : 1.0, xv, rv, zv, acc);
  if (WX) v.x[i] = xv;
  v.r[i] = rv; v.z[i] = zv;
}
// the step length from the host
struct CGUpdateF {
  double a;
  CGVecs v;
  template <int NOUT_>
  __device__ __forceinline__ void sweep(size_t tid, size_t stride, size_t n2, double (&acc)[NOUT_]) const { cg_sweep<true>(v, a, tid, stride, n2, acc); }
  __device__ void accum1(size_t i, double (&acc)[3]) const { cg_accum1<true>(v, a, i, acc); }
};
// The same sweep with the step length computed on the device: a = beta / dpi where dpi = p'w is still in device memory
// (the VecTDot kernel, all-reduced in place over RCCL on several ranks, wrote it there), so the host does not have to
// wait for the dot before it can launch the update -- one host synchronisation per CG iteration instead of two.
// KSPSolve_CG's break-down tests on dpi (cg.c:196-199) are evaluated here too (CGStepLen): when one fires nothing is
// modified, and the host, which receives dpi in out[3], takes the reference's exit with x, r, z untouched.  out[3] carries
// dpi through the reduction tree unchanged but for the sign of a zero (lane 0 of workgroup 0 contributes it, every other lane +0.0).
// x == NULL: the form without x and p (WX == false).
struct CGUpdateDevF {
  CGStepLen sl;
  CGVecs v;
  __device__ __forceinline__ void prologue(size_t tid, double (&acc)[4]) const {
    if (tid == 0) acc[3] = *sl.dpi_ptr;
  }
  template <int NOUT_>
  __device__ __forceinline__ void sweep(size_t tid, size_t stride, size_t n2, double (&acc)[NOUT_]) const {
    double a;
    if (!sl(a)) return;
    if (v.x) cg_sweep<true>(v, a, tid, stride, n2, acc);
    else cg_sweep<false>(v, a, tid, stride, n2, acc);
  }
  __device__ void accum1(size_t i, double (&acc)[4]) const {
    double a;
    if (!sl(a)) return;
    if (v.x) cg_accum1<true>(v, a, i, acc);
    else cg_accum1<false>(v, a, i, acc);
  }
};
template <> struct has_prologue<CGUpdateDevF> { static constexpr bool value = true; };

// ---- fused forms for KSPSolve_BCGS (bcgs.c:43-160); each keeps the element-wise arithmetic of the calls it replaces and
// the per-lane summation order of DotF / DotNorm2F / SumSqF under launch_reduce, so results carry the same bits.
// w = x .* d (PCApply_Jacobi; d == NULL: identity, PCNONE's copy) and Sum w*y (VecDot(w, y)): 4 passes instead of 5.
struct PMultDotF {
  const double *x, *d, *y;
  double *w;
  DEFAULT_SWEEP()
  __device__ void accum1(size_t i, double (&a)[1]) const {
    const double wv = x[i] * (d ? d[i] : 1.0);
    w[i] = wv;
    a[0] += wv * y[i];
  }
  __device__ void accum2(size_t i, double (&a)[1]) const {
    const double2 one2 = {1.0, 1.0};
    double2 xv = reinterpret_cast<const double2 *>(x)[i], dv = d ? reinterpret_cast<const double2 *>(d)[i] : one2;
    double2 yv = reinterpret_cast<const double2 *>(y)[i], wv;
    wv.x = xv.x * dv.x; wv.y = xv.y * dv.y;
    reinterpret_cast<double2 *>(w)[i] = wv;
    a[0] += wv.x * yv.x;
    a[0] += wv.y * yv.y;
  }
};
// w = x .* d and VecDotNorm2(s, w): Sum s*w, Sum w*w
struct PMultDotNorm2F {
  const double *x, *d, *s;
  double *w;
  DEFAULT_SWEEP()
  __device__ void accum1(size_t i, double (&a)[2]) const {
    const double wv = x[i] * (d ? d[i] : 1.0);
    w[i] = wv;
    a[0] += s[i] * wv; a[1] += wv * wv;
  }
  __device__ void accum2(size_t i, double (&a)[2]) const {
    const double2 one2 = {1.0, 1.0};
    double2 xv = reinterpret_cast<const double2 *>(x)[i], dv = d ? reinterpret_cast<const double2 *>(d)[i] : one2;
    double2 sv = reinterpret_cast<const double2 *>(s)[i], wv;
    wv.x = xv.x * dv.x; wv.y = xv.y * dv.y;
    reinterpret_cast<double2 *>(w)[i] = wv;
    a[0] += sv.x * wv.x; a[1] += wv.x * wv.x;
    a[0] += sv.y * wv.y; a[1] += wv.y * wv.y;
  }
};
// x = alpha p + omega s + x (VecAXPBYPCZ, gamma == 1 form, bvec1.c:436), r = s + (-omega) t (VecWAXPY, dvec2.c:1094),
// Sum r*r (VecNorm), Sum r*rp (next iteration's VecDot(R,RP)): 7 passes instead of 10, one reduction instead of two
struct BcgsUpdateF {
  double alpha, omega, momega;
  const double *p, *s, *t, *rp;
  double *x, *r;
  DEFAULT_SWEEP()
  __device__ __forceinline__ void one(double pv, double sv, double tv, double rpv, double &xv, double &rv, double (&a)[2]) const {
    xv = alpha * pv + omega * sv + xv;
    rv = (momega == 0.0) ? sv : sv + momega * tv;      // VecWAXPY copies for alpha == 0
    a[0] += rv * rv;
    a[1] += rv * rpv;
  }
  __device__ void accum1(size_t i, double (&a)[2]) const {
    double xv = x[i], rv;
    one(p[i], s[i], t[i], rp[i], xv, rv, a);
    x[i] = xv; r[i] = rv;
  }
  __device__ void accum2(size_t i, double (&a)[2]) const {
    // x is touched here only, s and t have their last reader here: streaming accesses (see nt_load2)
    double2 pv = reinterpret_cast<const double2 *>(p)[i], sv = nt_load2(reinterpret_cast<const double2 *>(s) + i);
    double2 tv = nt_load2(reinterpret_cast<const double2 *>(t) + i), qv = reinterpret_cast<const double2 *>(rp)[i];
    double2 xv = nt_load2(reinterpret_cast<double2 *>(x) + i), rv;
    one(pv.x, sv.x, tv.x, qv.x, xv.x, rv.x, a);
    one(pv.y, sv.y, tv.y, qv.y, xv.y, rv.y, a);
    nt_store2(reinterpret_cast<double2 *>(x) + i, xv);
    reinterpret_cast<double2 *>(r)[i] = rv;
  }
};

// ---- one step of KSPSolve_Chebychev (cheby.c) or KSPSolve_Richardson (rich.c) behind the product w = A p, KSP_NORM_NONE's whole
// iteration besides that product.  The residual, the diagonal preconditioner and the update in one sweep:
//   rv = b - w                (VecAYPX(r, -1, b) on r = w: OpXmY);     b == NULL: w is the preconditioned residual itself, zv = w
//   zv = rv * d               (PCApply_Jacobi: OpMul;  d == NULL: PCNONE's copy)
//   Chebyshev:   o = s zv + a pm + c pk     (VecScale, VecAXPY, VecAXPY with their special cases: OpScale, OpAxpy, OpAxpy)
//   Richardson:  o = o + s zv               (VecAXPY: OpAxpy)
// Each product and each sum is rounded as in those kernels, and with sums a lane meets its elements in SumSqF's order under
// launch_reduce: every output carries the bits of the separate launches.  An operand a special case skips is not loaded.
// Streaming (see nt_load2): b, d and pm have their only reader of the iteration here and r, z (when somebody wants them stored) no
// reader soon: non-temporal at every size, as the CG sweep treats d, x and r.  w (just written by the product), pk (next
// iteration's pm) and o (gathered by the next product) stay cacheable below 256 MiB and are streamed from there on like every
// other tile kernel.  A choice by analogy with the CG sweep: DESIGN.md has what was measured.
struct KrylovStepF {
  double s, a, c;
  const double *w, *b, *d, *pm, *pk;
  double *r, *z, *o;
  int rich, big;
  __device__ __forceinline__ void one(double wv, double bv, double dv, double pmv, double pkv, double &rv, double &zv, double &ov) const {
    rv = b ? bv - wv : wv;
    zv = d ? rv * dv : rv;
    if (rich) { ov = (s == 0.0) ? ov : ov + s * zv; return; }          // VecAXPY returns at once for alpha == 0 (bvec1.c:253)
    double t = (s == 1.0) ? zv : ((s == 0.0) ? 0.0 : s * zv);          // VecScale_Seq (bvec1.c:183): 1 -> nothing, 0 -> VecSet(0)
    t = (a == 0.0) ? t : t + a * pmv;
    ov = (c == 0.0) ? t : t + c * pkv;
  }
  // which operands this form reads (uniform over the launch)
  __device__ __forceinline__ bool reads_pm() const { return !rich && a != 0.0; }
  __device__ __forceinline__ bool reads_pk() const { return !rich && c != 0.0; }
  __device__ __forceinline__ bool reads_o() const { return rich && s != 0.0; }
  __device__ __forceinline__ bool writes_o() const { return !rich || s != 0.0; }
  // the U double2's of a lane in its tile; every load is issued before the first store, so r may be w and (b == NULL) o may be w
  template <bool BIG, int U>
  __device__ __forceinline__ void tile(size_t i, double2 (&rv)[U], double2 (&zv)[U]) const {
    double2 wv[U], bv[U] = {}, dv[U] = {}, pmv[U] = {}, pkv[U] = {}, ov[U] = {};
    ld_tile<BIG>(reinterpret_cast<const double2 *>(w), i, wv);
    if (b) ld_tile<true>(reinterpret_cast<const double2 *>(b), i, bv);
    if (d) ld_tile<true>(reinterpret_cast<const double2 *>(d), i, dv);
    if (reads_pm()) ld_tile<true>(reinterpret_cast<const double2 *>(pm), i, pmv);
    if (reads_pk()) ld_tile<BIG>(reinterpret_cast<const double2 *>(pk), i, pkv);
    if (reads_o()) ld_tile<BIG>(reinterpret_cast<const double2 *>(o), i, ov);
#pragma unroll
    for (int j = 0; j < U; ++j) {
      one(wv[j].x, bv[j].x, dv[j].x, pmv[j].x, pkv[j].x, rv[j].x, zv[j].x, ov[j].x);
      one(wv[j].y, bv[j].y, dv[j].y, pmv[j].y, pkv[j].y, rv[j].y, zv[j].y, ov[j].y);
    }
    if (r) st_tile<true>(reinterpret_cast<double2 *>(r), i, rv);
    if (z) st_tile<true>(reinterpret_cast<double2 *>(z), i, zv);
    if (writes_o()) st_tile<BIG>(reinterpret_cast<double2 *>(o), i, ov);
  }
  __device__ __forceinline__ void at1(size_t k, double &rv, double &zv) const {
    double ov = reads_o() ? o[k] : 0.0;
    one(w[k], b ? b[k] : 0.0, d ? d[k] : 0.0, reads_pm() ? pm[k] : 0.0, reads_pk() ? pk[k] : 0.0, rv, zv, ov);
    if (r) r[k] = rv;
    if (z) z[k] = zv;
    if (writes_o()) o[k] = ov;
  }
  // under launch_reduce: out = { sum zv*zv, sum rv*rv }, the trees of mi355x_vec_norm(type 1) over z and over r
  template <int NOUT_>
  __device__ __forceinline__ void sweep(size_t tid, size_t stride, size_t n2, double (&acc)[NOUT_]) const {
    for (size_t i = tid; i < n2; i += stride) {
      double2 rv[1], zv[1];
      if (big) tile<true, 1>(i, rv, zv); else tile<false, 1>(i, rv, zv);
      acc[0] += zv[0].x * zv[0].x; acc[1] += rv[0].x * rv[0].x;
      acc[0] += zv[0].y * zv[0].y; acc[1] += rv[0].y * rv[0].y;
    }
  }
  __device__ __forceinline__ void accum1(size_t k, double (&acc)[2]) const {
    double rv, zv;
    at1(k, rv, zv);
    acc[0] += zv * zv; acc[1] += rv * rv;
  }
};
// the same body as a pure map: one tile of 256 x 2 double2 per workgroup, nothing reduced
template <bool BIG>
__global__ __launch_bounds__(MI355X_BLOCK) void krylov_step_kernel(KrylovStepF f, size_t n, int vec_ok) {
  tile_walk<2>(n, vec_ok,
    [&](size_t i, auto u) {
      constexpr int U = decltype(u)::value;
      double2 rv[U], zv[U];
      f.template tile<BIG, U>(i, rv, zv);
    },
    [&](size_t k) { double rv, zv; f.at1(k, rv, zv); });
}
static int launch_krylov_step(mi355x_handle_t h, size_t n, KrylovStepF f, int sums, double *out) {
  const int vec_ok = all_aligned16(f.w, f.b, f.d, f.pm, f.pk, f.r, f.z, f.o);   // an operand the form does not touch is NULL
  f.big = vec_streams(n);
  if (sums) return launch_reduce<2, RED_SUM>(h, f, n, vec_ok, out);             // n == 0: zeros
  if (n == 0) return 0;
  return launch_tiles(h, n, vec_ok, krylov_step_kernel<true>, krylov_step_kernel<false>, f);
}

// ---- the body of KSPSolve_PIPECG's loop (pipecg.c:138-175) after the reduction has ended, behind m = B w and n = A m.  In one sweep:
//   zrec = nv + ratio zrec ; qrec = mv + ratio qrec ; p = u + ratio p ; s = w + ratio s      (VecAYPX x4: OpAypx with mi355x_vec_aypx's
//                                                        special cases 0 -> copy, 1 -> OpAxpy{1}, -1 -> OpXmY; first: VecCopy x4, nothing old read)
//   x = x + step p ; u = u + (-step) qrec ; w = w + (-step) zrec ; r = r + (-step) s         (VecAXPY x4: OpAxpy; step == 0: the four untouched)
//   m_next = w .* d                                      (PCApply_Jacobi: OpMul; d == NULL: PCNONE's copy; m_next == NULL: not formed)
//   out = { sum w*u , sum r*r | sum u*u | sum r*u }      (the next iteration's VecDot(w, u) and what rides with it)
// Each product and sum is rounded as in those kernels and with sums a lane meets its elements in DotF's / SumSqF's order under
// launch_reduce: every output carries the bits of the separate launches.  An operand a special case skips is not loaded.
// Streaming (see nt_load2), a choice by analogy with KrylovStepF, not a measurement: d, the four recurrences, x, u and r
// have their only reader of the iteration here and are non-temporal at every size; so is w when the preconditioner rides along
// (m_next), else PCApply reads it next.  nv (just written by the product), mv and m_next (gathered by the next product) stay
// cacheable below 256 MiB and are streamed from there on like every other tile kernel.
__device__ __forceinline__ void ldq_tile1(const double *p, size_t i, int nt, double2 &v) { v = ldq(reinterpret_cast<const double2 *>(p) + i, nt); }
template <int U> __device__ __forceinline__ void ldq_tile(const double *p, size_t i, int nt, double2 (&v)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u) ldq_tile1(p, i + u * MI355X_BLOCK, nt, v[u]);
}
template <int U> __device__ __forceinline__ void stq_tile(double *p, size_t i, int nt, const double2 (&v)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u) stq(reinterpret_cast<double2 *>(p) + i + u * MI355X_BLOCK, v[u], nt);
}
// y_new of VecAYPX(y, ratio, x) with the special cases of mi355x_vec_aypx; copy: VecCopy, or ratio == 0
__device__ __forceinline__ double aypx_elem(bool copy, double ratio, double xv, double yv) {
  if (copy) return xv;
  if (ratio == 1.0) return OpAxpy{1.0}(xv, yv, 0.0);
  if (ratio == -1.0) return OpXmY{}(xv, yv, 0.0);
  return OpAypx{ratio}(xv, yv, 0.0);
}
struct PipeCGStepF {
  double ratio, step;
  const double *nv, *mv, *d;
  double *zrec, *qrec, *p, *s, *x, *u, *w, *r, *m_next;
  int first, rides, big;       // rides: what the second sum is (1 r*r, 2 u*u, 3 r*u; 0: no sums at all)
  // which operands this form reads or writes (uniform over the launch)
  __device__ __forceinline__ bool copies() const { return first || ratio == 0.0; }
  __device__ __forceinline__ bool steps() const { return step != 0.0; }
  __device__ __forceinline__ bool reads_r() const { return steps() || rides == 1 || rides == 3; }
  __device__ __forceinline__ int w_nt() const { return big || m_next != nullptr; }
  __device__ __forceinline__ void one(double nvv, double mvv, double dv, double &zr, double &qr, double &pv, double &sv, double &xv, double &uv,
                                      double &wv, double &rv, double &mn) const {
    const bool cp = copies();
    zr = aypx_elem(cp, ratio, nvv, zr); qr = aypx_elem(cp, ratio, mvv, qr);
    pv = aypx_elem(cp, ratio, uv, pv); sv = aypx_elem(cp, ratio, wv, sv);
    if (steps()) {                                                   // VecAXPY returns at once for alpha == 0 (bvec1.c:253)
      xv = OpAxpy{step}(pv, xv, 0.0); uv = OpAxpy{-step}(qr, uv, 0.0);
      wv = OpAxpy{-step}(zr, wv, 0.0); rv = OpAxpy{-step}(sv, rv, 0.0);
    }
    mn = d ? OpMul{}(wv, dv, 0.0) : wv;
  }
  __device__ __forceinline__ void sums(double uv, double wv, double rv, double (&acc)[2]) const {
    acc[0] += wv * uv;
    acc[1] += rides == 1 ? rv * rv : (rides == 2 ? uv * uv : rv * uv);
  }
  // the U double2's of a lane in its tile; every load is issued before the first store, so m_next may be mv
  template <int U>
  __device__ __forceinline__ void tile(size_t i, double2 (&uv)[U], double2 (&wv)[U], double2 (&rv)[U]) const {
    double2 nvv[U], mvv[U], dv[U] = {}, zr[U] = {}, qr[U] = {}, pv[U] = {}, sv[U] = {}, xv[U] = {}, mn[U];
    ldq_tile(nv, i, big, nvv);
    ldq_tile(mv, i, big, mvv);
    if (d && m_next) ldq_tile(d, i, 1, dv);
    if (!copies()) { ldq_tile(zrec, i, 1, zr); ldq_tile(qrec, i, 1, qr); ldq_tile(p, i, 1, pv); ldq_tile(s, i, 1, sv); }
    if (steps()) ldq_tile(x, i, 1, xv);
    ldq_tile(u, i, 1, uv);
    ldq_tile(w, i, w_nt(), wv);
    if (reads_r()) ldq_tile(r, i, 1, rv);
#pragma unroll
    for (int j = 0; j < U; ++j) {
      one(nvv[j].x, mvv[j].x, dv[j].x, zr[j].x, qr[j].x, pv[j].x, sv[j].x, xv[j].x, uv[j].x, wv[j].x, rv[j].x, mn[j].x);
      one(nvv[j].y, mvv[j].y, dv[j].y, zr[j].y, qr[j].y, pv[j].y, sv[j].y, xv[j].y, uv[j].y, wv[j].y, rv[j].y, mn[j].y);
    }
    stq_tile(zrec, i, 1, zr); stq_tile(qrec, i, 1, qr); stq_tile(p, i, 1, pv); stq_tile(s, i, 1, sv);
    if (steps()) { stq_tile(x, i, 1, xv); stq_tile(u, i, 1, uv); stq_tile(w, i, w_nt(), wv); stq_tile(r, i, 1, rv); }
    if (m_next) stq_tile(m_next, i, big, mn);
  }
  __device__ __forceinline__ void at1(size_t k, double &uv, double &wv, double &rv) const {
    const bool cp = copies();
    const double nvv = nv[k], mvv = mv[k], dv = (d && m_next) ? d[k] : 0.0;
    double zr = cp ? 0.0 : zrec[k], qr = cp ? 0.0 : qrec[k], pv = cp ? 0.0 : p[k], sv = cp ? 0.0 : s[k], xv = steps() ? x[k] : 0.0, mn;
    uv = u[k]; wv = w[k]; rv = reads_r() ? r[k] : 0.0;
    one(nvv, mvv, dv, zr, qr, pv, sv, xv, uv, wv, rv, mn);
    zrec[k] = zr; qrec[k] = qr; p[k] = pv; s[k] = sv;
    if (steps()) { x[k] = xv; u[k] = uv; w[k] = wv; r[k] = rv; }
    if (m_next) m_next[k] = mn;
  }
  // under launch_reduce: the trees of mi355x_vec_dot / mi355x_vec_norm(type 1) over the updated vectors
  template <int NOUT_>
  __device__ __forceinline__ void sweep(size_t tid, size_t stride, size_t n2, double (&acc)[NOUT_]) const {
    for (size_t i = tid; i < n2; i += stride) {
      double2 uv[1], wv[1], rv[1] = {};
      tile<1>(i, uv, wv, rv);
      sums(uv[0].x, wv[0].x, rv[0].x, acc);
      sums(uv[0].y, wv[0].y, rv[0].y, acc);
    }
  }
  __device__ __forceinline__ void accum1(size_t k, double (&acc)[2]) const {
    double uv, wv, rv;
    at1(k, uv, wv, rv);
    sums(uv, wv, rv, acc);
  }
};
// the same body as a pure map: one tile of 256 x 2 double2 per workgroup, nothing reduced
__global__ __launch_bounds__(MI355X_BLOCK) void pipecg_step_kernel(PipeCGStepF f, size_t n, int vec_ok) {
  tile_walk<2>(n, vec_ok,
    [&](size_t i, auto u) {
      constexpr int U = decltype(u)::value;
      double2 uv[U], wv[U], rv[U] = {};
      f.template tile<U>(i, uv, wv, rv);
    },
    [&](size_t k) { double uv, wv, rv; f.at1(k, uv, wv, rv); });
}

// ---- the two sweeps of a MINRES iteration (KSPSolve_MINRES, src/ksp/ksp/impls/minres/minres.c) behind r = A u and alpha = u'r.
// MinresLanczosF, under launch_reduce:
//   z = r .* d                                           (PCApply_Jacobi: OpMul; d == NULL: z is taken as given)
//   r = r + (-alpha) v ; z = z + (-alpha) u ; r = r + (-beta) vold ; z = z + (-beta) uold     (VecAXPY x4 in this order: OpAxpy;
//                                                        alpha == 0 / beta == 0: that pair is skipped, as mi355x_vec_axpy returns at once)
//   out = { sum r*z , alpha }                            (VecDot(r, z) over the updated vectors; alpha rides home as lane 0's only term)
// alpha comes from the host or, alpha_dev != NULL, from the device slot the dot before left it in.  Each product and sum is rounded as
// in those kernels and a lane meets its elements in DotF's order: every output carries the bits of the separate launches.  An operand a
// special case skips is not loaded, a vector no case changes is not stored.
// Streaming (see nt_load2), a choice by analogy with PipeCGStepF, not a measurement: d, vold and uold have their only reader
// of the iteration here (the update sweep overwrites the two buffers) and are non-temporal at every size; r (just written by the
// product), z, v and u (read again by the update sweep or the next Lanczos sweep) stay cacheable below 256 MiB and are streamed from
// there on like every other tile kernel.
__device__ __forceinline__ double scale_elem(double al, double xv) {      // mi355x_vec_scale's cases: 0 -> VecSet(0), 1 -> nothing
  return al == 0.0 ? 0.0 : (al == 1.0 ? xv : OpScale{al}(xv, 0.0, 0.0));
}
struct MinresLanczosF {
  double alpha, beta;
  const double *alpha_dev, *d, *v, *u, *vold, *uold;
  double *r, *z;
  int big;
  __device__ __forceinline__ double al() const { return alpha_dev ? *alpha_dev : alpha; }
  __device__ __forceinline__ void prologue(size_t tid, double (&acc)[2]) const {
    if (tid == 0) acc[1] = al();
  }
  __device__ __forceinline__ void one(double a, double dv, double vv, double uv, double vo, double uo, double &rv, double &zv) const {
    if (d) zv = OpMul{}(rv, dv, 0.0);
    if (a != 0.0) { rv = OpAxpy{-a}(vv, rv, 0.0); zv = OpAxpy{-a}(uv, zv, 0.0); }
    if (beta != 0.0) { rv = OpAxpy{-beta}(vo, rv, 0.0); zv = OpAxpy{-beta}(uo, zv, 0.0); }
  }
  __device__ __forceinline__ void at2(size_t i, double a, double2 &rv, double2 &zv) const {
    double2 dv = {}, vv = {}, uv = {}, vo = {}, uo = {};
    zv = double2{};
    ldq_tile1(r, i, big, rv);
    if (d) ldq_tile1(d, i, 1, dv); else ldq_tile1(z, i, big, zv);
    if (a != 0.0) { ldq_tile1(v, i, big, vv); ldq_tile1(u, i, big, uv); }
    if (beta != 0.0) { ldq_tile1(vold, i, 1, vo); ldq_tile1(uold, i, 1, uo); }
    one(a, dv.x, vv.x, uv.x, vo.x, uo.x, rv.x, zv.x);
    one(a, dv.y, vv.y, uv.y, vo.y, uo.y, rv.y, zv.y);
    const bool moved = a != 0.0 || beta != 0.0;
    if (moved) stq(reinterpret_cast<double2 *>(r) + i, rv, big);
    if (moved || d) stq(reinterpret_cast<double2 *>(z) + i, zv, big);
  }
  __device__ __forceinline__ void at1(size_t k, double a, double &rv, double &zv) const {
    rv = r[k]; zv = d ? 0.0 : z[k];
    one(a, d ? d[k] : 0.0, a != 0.0 ? v[k] : 0.0, a != 0.0 ? u[k] : 0.0, beta != 0.0 ? vold[k] : 0.0, beta != 0.0 ? uold[k] : 0.0, rv, zv);
    const bool moved = a != 0.0 || beta != 0.0;
    if (moved) r[k] = rv;
    if (moved || d) z[k] = zv;
  }
  template <int NOUT_>
  __device__ __forceinline__ void sweep(size_t tid, size_t stride, size_t n2, double (&acc)[NOUT_]) const {
    const double a = al();
    for (size_t i = tid; i < n2; i += stride) {
      double2 rv, zv;
      at2(i, a, rv, zv);
      acc[0] += rv.x * zv.x;
      acc[0] += rv.y * zv.y;
    }
  }
  __device__ __forceinline__ void accum1(size_t k, double (&acc)[2]) const {
    double rv, zv;
    at1(k, al(), rv, zv);
    acc[0] += rv * zv;
  }
};
template <> struct has_prologue<MinresLanczosF> { static constexpr bool value = true; };

// MinresUpdateF, a pure map (nothing reduced, no host wait):
//   wn = u ; wn = wn + (-rho2) w ; wn = wn + (-rho3) wold ; wn = irho1 wn     (VecCopy, VecAXPY x2 in this order, VecScale; wn is stored
//                                                        over wold: the caller rotates (WOOLD, WOLD, W) <- (WOLD, W, that buffer))
//   x = x + ceta wn                                      (VecAXPY; ceta == 0: x neither read nor written)
//   vnew = ibeta r ; unew = ibeta z                      (VecCopy + VecScale x2, into the buffers of the old VOLD / UOLD)
// first != 0, the solve start: the last line alone.  mi355x_vec_axpy's alpha == 0 and mi355x_vec_scale's 0 -> VecSet(0), 1 -> nothing
// are honoured, and an operand a special case skips is not loaded (irho1 == 0: none of u, w, wold).
// Streaming, by the same analogy: x, r and z have their only reader of the iteration here (the next product overwrites r, the next
// preconditioner z) and wold is read for the last time: non-temporal loads at every size, and so is x's store.  u and w (next
// iteration's UOLD and WOLD), the new W, vnew (read by the next Lanczos sweep) and unew (gathered by the next product) stay cacheable
// below 256 MiB.
struct MinresUpdateF {
  double rho2, rho3, irho1, ceta, ibeta;
  const double *u, *w, *r, *z;
  double *wold, *x, *vnew, *unew;
  int first, big;
  __device__ __forceinline__ bool reads_u() const { return !first && irho1 != 0.0; }
  __device__ __forceinline__ bool reads_w() const { return reads_u() && rho2 != 0.0; }
  __device__ __forceinline__ bool reads_wold() const { return reads_u() && rho3 != 0.0; }
  __device__ __forceinline__ bool steps() const { return !first && ceta != 0.0; }
  __device__ __forceinline__ bool reads_rz() const { return ibeta != 0.0; }
  __device__ __forceinline__ void one(double uv, double wv, double wo, double rv, double zv, double &wn, double &xv, double &vn, double &un) const {
    if (!first) {
      double t = uv;
      if (rho2 != 0.0) t = OpAxpy{-rho2}(wv, t, 0.0);
      if (rho3 != 0.0) t = OpAxpy{-rho3}(wo, t, 0.0);
      wn = scale_elem(irho1, t);
      if (ceta != 0.0) xv = OpAxpy{ceta}(wn, xv, 0.0);
    }
    vn = scale_elem(ibeta, rv); un = scale_elem(ibeta, zv);
  }
  // the U double2's of a lane in its tile; every load is issued before the first store
  template <int U>
  __device__ __forceinline__ void tile(size_t i) const {
    double2 uv[U] = {}, wv[U] = {}, wo[U] = {}, rv[U] = {}, zv[U] = {}, xv[U] = {}, wn[U] = {}, vn[U], un[U];
    if (reads_u()) ldq_tile(u, i, big, uv);
    if (reads_w()) ldq_tile(w, i, big, wv);
    if (reads_wold()) ldq_tile(wold, i, 1, wo);
    if (steps()) ldq_tile(x, i, 1, xv);
    if (reads_rz()) { ldq_tile(r, i, 1, rv); ldq_tile(z, i, 1, zv); }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      one(uv[j].x, wv[j].x, wo[j].x, rv[j].x, zv[j].x, wn[j].x, xv[j].x, vn[j].x, un[j].x);
      one(uv[j].y, wv[j].y, wo[j].y, rv[j].y, zv[j].y, wn[j].y, xv[j].y, vn[j].y, un[j].y);
    }
    if (!first) stq_tile(wold, i, big, wn);
    if (steps()) stq_tile(x, i, 1, xv);
    stq_tile(vnew, i, big, vn); stq_tile(unew, i, big, un);
  }
  __device__ __forceinline__ void at1(size_t k) const {
    double wn = 0.0, xv = steps() ? x[k] : 0.0, vn, un;
    one(reads_u() ? u[k] : 0.0, reads_w() ? w[k] : 0.0, reads_wold() ? wold[k] : 0.0, reads_rz() ? r[k] : 0.0, reads_rz() ? z[k] : 0.0, wn, xv, vn, un);
    if (!first) wold[k] = wn;
    if (steps()) x[k] = xv;
    vnew[k] = vn; unew[k] = un;
  }
};
__global__ __launch_bounds__(MI355X_BLOCK) void minres_update_kernel(MinresUpdateF f, size_t n, int vec_ok) {
  tile_walk<2>(n, vec_ok,
    [&](size_t i, auto u) { f.template tile<decltype(u)::value>(i); },
    [&](size_t k) { f.at1(k); });
}

// ---- the three sweeps of an iteration of KSPSolve_TFQMR (src/ksp/ksp/impls/tfqmr/tfqmr.c) and KSPSolve_CGS (src/ksp/ksp/impls/cgs/cgs.c),
// which share one skeleton, around the two applications of the preconditioned operator.  Each product and sum is rounded as in
// mi355x_vec_waxpy, _axpy and _aypx, whose scalar special cases are kept; an operand a special case skips is not loaded, a vector no case
// changes is not stored; under launch_reduce a lane meets its elements in SumSqF's / DotF's order: every output carries the bits of the
// separate launches.
// w of VecWAXPY(w, al, x, y) with the cases of mi355x_vec_waxpy (1, -1, 0 -> copy of y)
__device__ __forceinline__ double waxpy_elem(double al, double xv, double yv) {
  if (al == 1.0) return OpXpY{}(xv, yv, 0.0);
  if (al == -1.0) return OpYmX{}(xv, yv, 0.0);
  if (al == 0.0) return yv;
  return OpAxpy{al}(xv, yv, 0.0);
}
// TfqmrQTF, a pure map:
//   q = u + (-a) v                                       (VecWAXPY(Q, -a, V, U); a == 0: a copy of u, v not loaded)
//   t = q + u                                            (VecWAXPY(T, 1.0, U, Q): the alpha == 1 form)
//   x = x + a t                                          (CGS, x != NULL: VecAXPY(X, a, T); a == 0: x neither read nor written)
// Streaming (see nt_load2), a choice by analogy with the MINRES sweeps, not a measurement: v has its last reader here (the
// product that follows overwrites its buffer) and x is touched here only: non-temporal at every size; u and q (read again by the update
// sweep) and t (gathered by the product that follows) stay cacheable below 256 MiB and are streamed from there on like every other
// tile kernel.
struct TfqmrQTF {
  double a;
  const double *u, *v;
  double *q, *t, *x;
  int big;
  __device__ __forceinline__ bool reads_v() const { return a != 0.0; }
  __device__ __forceinline__ bool steps() const { return x != nullptr && a != 0.0; }
  __device__ __forceinline__ void one(double uv, double vv, double &qv, double &tv, double &xv) const {
    qv = waxpy_elem(-a, vv, uv);
    tv = OpXpY{}(uv, qv, 0.0);
    if (steps()) xv = OpAxpy{a}(tv, xv, 0.0);
  }
  template <int U>
  __device__ __forceinline__ void tile(size_t i) const {
    double2 uv[U], vv[U] = {}, xv[U] = {}, qv[U], tv[U];
    ldq_tile(u, i, big, uv);
    if (reads_v()) ldq_tile(v, i, 1, vv);
    if (steps()) ldq_tile(x, i, 1, xv);
#pragma unroll
    for (int j = 0; j < U; ++j) {
      one(uv[j].x, vv[j].x, qv[j].x, tv[j].x, xv[j].x);
      one(uv[j].y, vv[j].y, qv[j].y, tv[j].y, xv[j].y);
    }
    stq_tile(q, i, big, qv); stq_tile(t, i, big, tv);
    if (steps()) stq_tile(x, i, 1, xv);
  }
  __device__ __forceinline__ void at1(size_t k) const {
    double qv, tv, xv = steps() ? x[k] : 0.0;
    one(u[k], reads_v() ? v[k] : 0.0, qv, tv, xv);
    q[k] = qv; t[k] = tv;
    if (steps()) x[k] = xv;
  }
};
__global__ __launch_bounds__(MI355X_BLOCK) void tfqmr_qt_kernel(TfqmrQTF f, size_t n, int vec_ok) {
  tile_walk<2>(n, vec_ok,
    [&](size_t i, auto u) { f.template tile<decltype(u)::value>(i); },
    [&](size_t k) { f.at1(k); });
}

// TfqmrResidF, under launch_reduce:
//   r = r + (-a) auq                                     (VecAXPY(R, -a, AUQ); a == 0: r not stored, auq not loaded)
//   out = { sum r*r , sum r*rp }                         (VecNorm(R, NORM_2)'s sum and VecDot(R, RP) over the updated r)
// Streaming, by the same analogy: auq has its only reader here (the next product overwrites its buffer): non-temporal at every size;
// r (read again by the update sweep) and rp (read by every iteration's two reductions) stay cacheable below 256 MiB.
struct TfqmrResidF {
  double ma;                   // -a, the scalar VecAXPY is called with
  const double *auq, *rp;
  double *r;
  int big;
  __device__ __forceinline__ bool moves() const { return ma != 0.0; }
  template <int NOUT_>
  __device__ __forceinline__ void sweep(size_t tid, size_t stride, size_t n2, double (&acc)[NOUT_]) const {
    for (size_t i = tid; i < n2; i += stride) {
      double2 rv, pv, av = {};
      ldq_tile1(r, i, big, rv);
      ldq_tile1(rp, i, big, pv);
      if (moves()) {
        ldq_tile1(auq, i, 1, av);
        rv.x = OpAxpy{ma}(av.x, rv.x, 0.0); rv.y = OpAxpy{ma}(av.y, rv.y, 0.0);
        stq(reinterpret_cast<double2 *>(r) + i, rv, big);
      }
      acc[0] += rv.x * rv.x; acc[1] += rv.x * pv.x;
      acc[0] += rv.y * rv.y; acc[1] += rv.y * pv.y;
    }
  }
  __device__ __forceinline__ void accum1(size_t k, double (&acc)[2]) const {
    double rv = r[k];
    if (moves()) { rv = OpAxpy{ma}(auq[k], rv, 0.0); r[k] = rv; }
    acc[0] += rv * rv; acc[1] += rv * rp[k];
  }
};

// TfqmrUpdateF, a pure map (nothing reduced, no host wait):
//   nhalves >= 1:  d = u + cf0 d ; x = x + eta0 d        (VecAYPX(D, cf0, U), VecAXPY(X, eta0, D): the m = 0 half of TFQMR's inner loop)
//   nhalves == 2:  d = q + cf1 d ; x = x + eta1 d        (VecAYPX(D, cf1, Q), VecAXPY(X, eta1, D): the m = 1 half)
//   tail != 0:     un = r + b q ; qn = q + b p ; pn = un + b qn, stored to u, q, p
//                                                        (VecWAXPY(U, b, Q, R), VecAXPY(Q, b, P), VecWAXPY(P, b, Q, U))
// The halves read the OLD u and q: every operand is loaded before the first store.  mi355x_vec_aypx's cases (cf == 0: a copy, d not
// loaded; 1; -1), mi355x_vec_axpy's (eta == 0, b == 0: untouched) and mi355x_vec_waxpy's (b == 1, -1, 0: copies, q and p not loaded) are
// honoured.  nhalves == 0 (CGS) touches neither d nor x; tail == 0 (an exit inside TFQMR's inner loop) none of u, q, p, r.
// Streaming, by the same analogy: d and x are touched here only, the old u, q, p and r are read for the last time, and the new q has no
// reader at all (the next TfqmrQTF overwrites it): non-temporal at every size.  The new u (read by the next TfqmrQTF) and the new p
// (gathered by the product that follows) stay cacheable below 256 MiB.
struct TfqmrUpdateF {
  double cf0, eta0, cf1, eta1, b;
  const double *r;
  double *d, *x, *u, *q, *p;
  int nhalves, tail, big;
  __device__ __forceinline__ bool reads_d() const { return nhalves >= 1 && cf0 != 0.0; }
  __device__ __forceinline__ bool steps() const { return (nhalves >= 1 && eta0 != 0.0) || (nhalves == 2 && eta1 != 0.0); }
  __device__ __forceinline__ bool reads_u() const { return nhalves >= 1; }
  __device__ __forceinline__ bool moves_q() const { return tail && b != 0.0; }       // VecAXPY(Q, b, P) does something; p is read
  __device__ __forceinline__ bool reads_q() const { return nhalves == 2 || moves_q(); }
  __device__ __forceinline__ void one(double rv, double &dv, double &xv, double &uv, double &qv, double &pv) const {
    if (nhalves >= 1) {
      dv = aypx_elem(cf0 == 0.0, cf0, uv, dv);
      if (eta0 != 0.0) xv = OpAxpy{eta0}(dv, xv, 0.0);
    }
    if (nhalves == 2) {
      dv = aypx_elem(cf1 == 0.0, cf1, qv, dv);
      if (eta1 != 0.0) xv = OpAxpy{eta1}(dv, xv, 0.0);
    }
    if (tail) {
      uv = waxpy_elem(b, qv, rv);
      if (b != 0.0) qv = OpAxpy{b}(pv, qv, 0.0);
      pv = waxpy_elem(b, qv, uv);
    }
  }
  // the U double2's of a lane in its tile; every load is issued before the first store
  template <int U>
  __device__ __forceinline__ void tile(size_t i) const {
    double2 rv[U] = {}, dv[U] = {}, xv[U] = {}, uv[U] = {}, qv[U] = {}, pv[U] = {};
    if (reads_d()) ldq_tile(d, i, 1, dv);
    if (steps()) ldq_tile(x, i, 1, xv);
    if (reads_u()) ldq_tile(u, i, 1, uv);
    if (reads_q()) ldq_tile(q, i, 1, qv);
    if (tail) ldq_tile(r, i, 1, rv);
    if (moves_q()) ldq_tile(p, i, 1, pv);
#pragma unroll
    for (int j = 0; j < U; ++j) {
      one(rv[j].x, dv[j].x, xv[j].x, uv[j].x, qv[j].x, pv[j].x);
      one(rv[j].y, dv[j].y, xv[j].y, uv[j].y, qv[j].y, pv[j].y);
    }
    if (nhalves >= 1) stq_tile(d, i, 1, dv);
    if (steps()) stq_tile(x, i, 1, xv);
    if (tail) stq_tile(u, i, big, uv);
    if (moves_q()) stq_tile(q, i, 1, qv);
    if (tail) stq_tile(p, i, big, pv);
  }
  __device__ __forceinline__ void at1(size_t k) const {
    double dv = reads_d() ? d[k] : 0.0, xv = steps() ? x[k] : 0.0, uv = reads_u() ? u[k] : 0.0, qv = reads_q() ? q[k] : 0.0, pv = moves_q() ? p[k] : 0.0;
    one(tail ? r[k] : 0.0, dv, xv, uv, qv, pv);
    if (nhalves >= 1) d[k] = dv;
    if (steps()) x[k] = xv;
    if (tail) u[k] = uv;
    if (moves_q()) q[k] = qv;
    if (tail) p[k] = pv;
  }
};
__global__ __launch_bounds__(MI355X_BLOCK) void tfqmr_update_kernel(TfqmrUpdateF f, size_t n, int vec_ok) {
  tile_walk<2>(n, vec_ok,
    [&](size_t i, auto u) { f.template tile<decltype(u)::value>(i); },
    [&](size_t k) { f.at1(k); });
}

// ---- the two sweeps of an iteration of KSPSolve_BiCG (src/ksp/ksp/impls/bicg/bicg.c) around A pr, A^T pl and the preconditioner, over
// the shared steps above (aypx_elem, OpAxpy, the tile loads and stores); every output carries the bits of the separate launches.
// BicgDirsF, a pure map (nothing reduced, no host wait):
//   first:  pr = zr ; pl = zl                              (VecCopy x2)
//   else:   pr = zr + b pr ; pl = zl + b pl                (VecAYPX(Pr, b, Zr), VecAYPX(Pl, b, Zl); b == 0: copies, pr / pl not loaded; 1; -1)
// zr and zl have their last readers here (the two products that follow overwrite them): non-temporal at every size; the new pr and pl
// are gathered by those products and stay cacheable below 256 MiB.
struct BicgDirsF {
  double b;
  const double *zr, *zl;
  double *pr, *pl;
  int first, big;
  __device__ __forceinline__ bool copies() const { return first || b == 0.0; }
  template <int U>
  __device__ __forceinline__ void tile(size_t i) const {
    double2 zrv[U], zlv[U], prv[U] = {}, plv[U] = {};
    ldq_tile(zr, i, 1, zrv); ldq_tile(zl, i, 1, zlv);
    if (!copies()) { ldq_tile(pr, i, big, prv); ldq_tile(pl, i, big, plv); }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      prv[j].x = aypx_elem(copies(), b, zrv[j].x, prv[j].x); prv[j].y = aypx_elem(copies(), b, zrv[j].y, prv[j].y);
      plv[j].x = aypx_elem(copies(), b, zlv[j].x, plv[j].x); plv[j].y = aypx_elem(copies(), b, zlv[j].y, plv[j].y);
    }
    stq_tile(pr, i, big, prv); stq_tile(pl, i, big, plv);
  }
  __device__ __forceinline__ void at1(size_t k) const {
    pr[k] = aypx_elem(copies(), b, zr[k], copies() ? 0.0 : pr[k]);
    pl[k] = aypx_elem(copies(), b, zl[k], copies() ? 0.0 : pl[k]);
  }
};
__global__ __launch_bounds__(MI355X_BLOCK) void bicg_dirs_kernel(BicgDirsF f, size_t n, int vec_ok) {
  tile_walk<2>(n, vec_ok,
    [&](size_t i, auto u) { f.template tile<decltype(u)::value>(i); },
    [&](size_t k) { f.at1(k); });
}

// BicgUpdateF, under launch_reduce:
//   x = x + a pr ; rr = rr + (-a) zr ; rl = rl + (-a) zl   (VecAXPY x3; a == 0: nothing moved, pr / zr / zl not loaded as inputs)
//   pcmode 1 (PCJACOBI): zr = rr * d ; zl = rl * d         (VecPointwiseMult(Zr, Rr, diag), (Zl, Rl, diag): a diagonal is its own transpose)
//   pcmode 2 (PCNONE):   zr = rr ; zl = rl                 (VecCopy x2)
//   pcmode 0:            zr and zl are left to the caller's PCApply / PCApplyTranspose
//   out = { sum zr*rl , sum zr*zr or sum rr*rr }           (VecDot(Zr, Rl) = the next beta; VecNorm(Zr or Rr, NORM_2)'s sum, by `which`);
//                                                          pcmode 0: { 0 , sum rr*rr }
// over the updated vectors, a lane meeting its elements in DotF's / SumSqF's order.  x is touched here only and the old zr / zl are read
// for the last time: non-temporal at every size; rr, rl and the new zr, zl stay cacheable below 256 MiB.
struct BicgUpdateF {
  double a;
  const double *pr, *d;
  double *x, *rr, *rl, *zr, *zl;
  int pcmode, which, big;      // which: 0 the sum of zr*zr, 1 of rr*rr
  __device__ __forceinline__ bool moves() const { return a != 0.0; }
  __device__ __forceinline__ void one(double prv, double dv, double &xv, double &rrv, double &rlv, double &zrv, double &zlv, double (&acc)[2]) const {
    if (moves()) {
      xv = OpAxpy{a}(prv, xv, 0.0);
      rrv = OpAxpy{-a}(zrv, rrv, 0.0);
      rlv = OpAxpy{-a}(zlv, rlv, 0.0);
    }
    if (pcmode == 1) { zrv = rrv * dv; zlv = rlv * dv; }
    else if (pcmode == 2) { zrv = rrv; zlv = rlv; }
    if (pcmode) acc[0] += zrv * rlv;
    if (pcmode && !which) acc[1] += zrv * zrv;
    else acc[1] += rrv * rrv;
  }
  template <int NOUT_>
  __device__ __forceinline__ void sweep(size_t tid, size_t stride, size_t n2, double (&acc)[NOUT_]) const {
    for (size_t i = tid; i < n2; i += stride) {
      double2 xv = {}, prv = {}, rrv, rlv, zrv = {}, zlv = {}, dv = {};
      ldq_tile1(rr, i, big, rrv); ldq_tile1(rl, i, big, rlv);
      if (moves()) { ldq_tile1(x, i, 1, xv); ldq_tile1(pr, i, 1, prv); ldq_tile1(zr, i, 1, zrv); ldq_tile1(zl, i, 1, zlv); }
      if (pcmode == 1) ldq_tile1(d, i, big, dv);
      one(prv.x, dv.x, xv.x, rrv.x, rlv.x, zrv.x, zlv.x, acc);
      one(prv.y, dv.y, xv.y, rrv.y, rlv.y, zrv.y, zlv.y, acc);
      if (moves()) {
        stq(reinterpret_cast<double2 *>(x) + i, xv, 1);
        stq(reinterpret_cast<double2 *>(rr) + i, rrv, big); stq(reinterpret_cast<double2 *>(rl) + i, rlv, big);
      }
      if (pcmode) { stq(reinterpret_cast<double2 *>(zr) + i, zrv, big); stq(reinterpret_cast<double2 *>(zl) + i, zlv, big); }
    }
  }
  __device__ __forceinline__ void accum1(size_t k, double (&acc)[2]) const {
    double xv = 0.0, prv = 0.0, rrv = rr[k], rlv = rl[k], zrv = 0.0, zlv = 0.0;
    if (moves()) { xv = x[k]; prv = pr[k]; zrv = zr[k]; zlv = zl[k]; }
    one(prv, pcmode == 1 ? d[k] : 0.0, xv, rrv, rlv, zrv, zlv, acc);
    if (moves()) { x[k] = xv; rr[k] = rrv; rl[k] = rlv; }
    if (pcmode) { zr[k] = zrv; zl[k] = zlv; }
  }
};

// ---- the two sweeps of an LSQR iteration (the Golub-Kahan bidiagonalisation of KSPSolve_LSQR, src/ksp/ksp/impls/lsqr/lsqr.c) around the
// products u1 = A v and v1 = A^T u1.
// LsqrBidiagF, under launch_reduce:
//   y = y + (-coef) x                                    (VecAXPY(Y, -coef, X): OpAxpy; coef == 0: y not stored, x not loaded)
//   out = sum y*y                                        (VecNorm(Y, NORM_2)'s sum over the updated y; a lane meets its elements in SumSqF's order)
// coef comes from the host or, coef2_dev != NULL, is sqrt(*coef2_dev) formed on the device: the sum the same sweep left in a device slot
// one product earlier, rooted as the host roots it (IEEE sqrt is correctly rounded on both sides).
// Streaming (see nt_load2), a choice by analogy with TfqmrResidF, not a measurement: x (the previous u or v) has its last
// reader of the iteration here -- the next product overwrites its buffer -- and is non-temporal at every size; y (just written by the
// product, read again by the scaling or the update sweep and gathered by the next product) stays cacheable below 256 MiB.
struct LsqrBidiagF {
  double coef;
  const double *coef2_dev, *x;
  double *y;
  int big;
  __device__ __forceinline__ double ma() const { return -(coef2_dev ? sqrt(*coef2_dev) : coef); }   // the scalar VecAXPY is called with
  template <int NOUT_>
  __device__ __forceinline__ void sweep(size_t tid, size_t stride, size_t n2, double (&acc)[NOUT_]) const {
    const double a = ma();
    for (size_t i = tid; i < n2; i += stride) {
      double2 yv, xv;
      ldq_tile1(y, i, big, yv);
      if (a != 0.0) {
        ldq_tile1(x, i, 1, xv);
        yv.x = OpAxpy{a}(xv.x, yv.x, 0.0); yv.y = OpAxpy{a}(xv.y, yv.y, 0.0);
        stq(reinterpret_cast<double2 *>(y) + i, yv, big);
      }
      acc[0] += yv.x * yv.x;
      acc[0] += yv.y * yv.y;
    }
  }
  __device__ __forceinline__ void accum1(size_t k, double (&acc)[1]) const {
    const double a = ma();
    double yv = y[k];
    if (a != 0.0) { yv = OpAxpy{a}(x[k], yv, 0.0); y[k] = yv; }
    acc[0] += yv * yv;
  }
};

// LsqrUpdateF, a pure map (nothing reduced, no host wait):
//   v1 = ialpha v1                                       (VecScale; 1: v1 not stored, 0: zeros and v1 not loaded)
//   x = x + step w                                       (VecAXPY; step == 0: x neither read nor written)
//   se = se + irho2 (w .* w)                             (se != NULL: VecCopy, VecPointwiseMult, VecScale, VecAXPY(1.0) through a scratch vector)
//   w = v1 + cf w                                        (VecAYPX with mi355x_vec_aypx's cases, over the SCALED v1 held in registers;
//                                                         skip_w: w not stored -- the breakdown exit, where x and se still take the old w)
// An operand no line of the form needs is not loaded.
// Streaming, by the same analogy: x and se are touched here only: non-temporal at every size; v1 (just written by the bidiagonalisation
// sweep, gathered by the next product) and w (read again by the next update) stay cacheable below 256 MiB.
struct LsqrUpdateF {
  double ialpha, step, cf, irho2;
  double *v1, *x, *w, *se;
  int skip_w, big;
  __device__ __forceinline__ bool reads_v1() const { return ialpha != 0.0 && (ialpha != 1.0 || !skip_w); }
  __device__ __forceinline__ bool writes_v1() const { return ialpha != 1.0; }
  __device__ __forceinline__ bool steps() const { return step != 0.0; }
  __device__ __forceinline__ bool reads_w() const { return steps() || se != nullptr || (!skip_w && cf != 0.0); }
  __device__ __forceinline__ void one(double &vv, double &xv, double &wv, double &sv) const {
    vv = scale_elem(ialpha, vv);
    if (steps()) xv = OpAxpy{step}(wv, xv, 0.0);
    if (se) sv = OpAxpy{1.0}(scale_elem(irho2, OpMul{}(wv, wv, 0.0)), sv, 0.0);
    if (!skip_w) wv = aypx_elem(cf == 0.0, cf, vv, wv);
  }
  // the U double2's of a lane in its tile; every load is issued before the first store
  template <int U>
  __device__ __forceinline__ void tile(size_t i) const {
    double2 vv[U] = {}, xv[U] = {}, wv[U] = {}, sv[U] = {};
    if (reads_v1()) ldq_tile(v1, i, big, vv);
    if (steps()) ldq_tile(x, i, 1, xv);
    if (reads_w()) ldq_tile(w, i, big, wv);
    if (se) ldq_tile(se, i, 1, sv);
#pragma unroll
    for (int j = 0; j < U; ++j) {
      one(vv[j].x, xv[j].x, wv[j].x, sv[j].x);
      one(vv[j].y, xv[j].y, wv[j].y, sv[j].y);
    }
    if (writes_v1()) stq_tile(v1, i, big, vv);
    if (steps()) stq_tile(x, i, 1, xv);
    if (se) stq_tile(se, i, 1, sv);
    if (!skip_w) stq_tile(w, i, big, wv);
  }
  __device__ __forceinline__ void at1(size_t k) const {
    double vv = reads_v1() ? v1[k] : 0.0, xv = steps() ? x[k] : 0.0, wv = reads_w() ? w[k] : 0.0, sv = se ? se[k] : 0.0;
    one(vv, xv, wv, sv);
    if (writes_v1()) v1[k] = vv;
    if (steps()) x[k] = xv;
    if (se) se[k] = sv;
    if (!skip_w) w[k] = wv;
  }
};
__global__ __launch_bounds__(MI355X_BLOCK) void lsqr_update_kernel(LsqrUpdateF f, size_t n, int vec_ok) {
  tile_walk<2>(n, vec_ok,
    [&](size_t i, auto u) { f.template tile<decltype(u)::value>(i); },
    [&](size_t k) { f.at1(k); });
}

template <int NV>
struct MDotF {
  const double *x;
  const double *y[NV];
  int nt;
  template <int NOUT_>
  __device__ __forceinline__ void sweep(size_t tid, size_t stride, size_t n2, double (&a)[NOUT_]) const {
    size_t i = tid;
    if (NV <= 4) for (; i + stride < n2; i += 2 * stride) { accum2(i, a); accum2(i + stride, a); }
    for (; i < n2; i += stride) accum2(i, a);
  }
  __device__ void accum1(size_t i, double (&a)[NV]) const {
    double xv = x[i];
#pragma unroll
    for (int j = 0; j < NV; ++j) a[j] += xv * y[j][i];
  }
  __device__ void accum2(size_t i, double (&a)[NV]) const {
    double2 xv = reinterpret_cast<const double2 *>(x)[i];
    double2 yv[NV];
    load_basis<NV>(y, i, nt, yv);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      a[j] += xv.x * yv[j].x;
      a[j] += xv.y * yv[j].y;
    }
  }
};


// ---- fused forms for KSPGMRESCycle (gmres.c:118-209) ------------------------------------------------------------------
// The Gram-Schmidt update x += sum_j (-h_j) y_j (VecMAXPY of borthog2.c:64 with the coefficients VecMDot has just left in
// device memory, negated as borthog2.c:63 does) and Sum x_new^2 (the VecNorm inside gmres.c:146's VecNormalize) in ONE
// sweep: the grouping of maxpy_elem (= petscaxpy.h:101-110) and the per-lane order of SumSqF, so x and the norm carry the
// bits of the separate calls.  Up to 32 vectors per sweep.
template <int G0, int NG4>
struct MaxpyNormF {
  static constexpr int NV = G0 + 4 * NG4;
  const double *y[NV];
  int nt;
  const double *adev;   // coefficients in device memory ...
  double sign;          // ... times +-1
  double *x;
  double a[NV];
  __device__ __forceinline__ void prologue(size_t, double (&)[1]) {
#pragma unroll
    for (int j = 0; j < NV; ++j) a[j] = sign * adev[j];   // (-1) * h: the bits of -h
  }
  template <int NOUT_>
  __device__ __forceinline__ void sweep(size_t tid, size_t stride, size_t n2, double (&acc)[NOUT_]) const {
    for (size_t i = tid; i < n2; i += stride) accum2(i, acc);
  }
  __device__ __forceinline__ void accum1(size_t i, double (&acc)[1]) const {
    const double xv = maxpy_at1<G0, NG4>(y, a, x, i);
    x[i] = xv;
    acc[0] += xv * xv;
  }
  __device__ __forceinline__ void accum2(size_t i, double (&acc)[1]) const {
    const double2 xv = maxpy_at2<G0, NG4>(y, a, nt, x, i);
    reinterpret_cast<double2 *>(x)[i] = xv;
    acc[0] += xv.x * xv.x;
    acc[0] += xv.y * xv.y;
  }
};
template <int G0, int NG4> struct has_prologue<MaxpyNormF<G0, NG4>> { static constexpr bool value = true; };

// x *= 1/sqrt(*norm2) with the cases of VecNormalize (rvector.c:308-314: a zero norm leaves x alone, so does a norm of one)
// and of VecScale_Seq (bvec1.c:183: alpha == 0 sets zero); sqrt and the division are IEEE-exact on the device as on the host
__global__ __launch_bounds__(MI355X_BLOCK) void scale_rnorm_dev_kernel(const double *norm2, double *x, size_t n, int vec_ok) {
  const double nrm = sqrt(*norm2);
  if (nrm == 0.0 || nrm == 1.0) return;
  const double alpha = 1.0 / nrm;
  if (alpha == 1.0) return;
  const auto scaled = [=](double v) { return alpha == 0.0 ? 0.0 : v * alpha; };
  double2 *x2 = reinterpret_cast<double2 *>(x);
  tile_walk<2>(n, vec_ok,
    [&](size_t i, auto u) {
      double2 v[decltype(u)::value];
      ld_tile<false>(x2, i, v);
      for (double2 &e : v) { e.x = scaled(e.x); e.y = scaled(e.y); }
      st_tile<false>(x2, i, v);
    },
    [&](size_t k) { x[k] = scaled(x[k]); });
}

// scale_rnorm_dev_kernel and, in the same pass, z = d .* x_new (d == NULL: z = x_new): gmres.c:146's VecNormalize followed by the
// PCApply_Jacobi / PCApply_None of the NEXT flexible-GMRES step (VecPointwiseMult / VecCopy), whose input is still in registers.
// x is stored under the rules above only (a norm of 0 or 1, alpha == 1: not stored); z is written for every entry.
__global__ __launch_bounds__(MI355X_BLOCK) void scale_rnorm_dev_pmult_kernel(const double *norm2, double *x, const double *d, double *z, size_t n, int vec_ok) {
  const double nrm = sqrt(*norm2);
  const double alpha = 1.0 / nrm;
  const bool keep = nrm == 0.0 || nrm == 1.0 || alpha == 1.0;
  const auto scaled = [=](double v) { return alpha == 0.0 ? 0.0 : v * alpha; };
  double2 *x2 = reinterpret_cast<double2 *>(x), *z2 = reinterpret_cast<double2 *>(z);
  const double2 *d2 = reinterpret_cast<const double2 *>(d);
  tile_walk<2>(n, vec_ok,
    [&](size_t i, auto u) {
      constexpr int U = decltype(u)::value;
      double2 v[U], dv[U] = {};
      ld_tile<false>(x2, i, v);
      if (d) ld_tile<false>(d2, i, dv);
      if (!keep) {
        for (double2 &e : v) { e.x = scaled(e.x); e.y = scaled(e.y); }
        st_tile<false>(x2, i, v);
      }
      if (d) {
#pragma unroll
        for (int j = 0; j < U; ++j) { v[j].x = v[j].x * dv[j].x; v[j].y = v[j].y * dv[j].y; }
      }
      st_tile<false>(z2, i, v);
    },
    [&](size_t k) {
      double v = x[k];
      if (!keep) { v = scaled(v); x[k] = v; }
      z[k] = d ? v * d[k] : v;
    });
}

template <int NV>
static int launch_mdot(mi355x_handle_t h, size_t n, const double *x, const double *const *y, double *out) {
  MDotF<NV> f;
  f.x = x;
  f.nt = gs_streams(n, NV);
  const int vec_ok = fill_basis(f.y, y, NV) && all_aligned16(x);
  return launch_reduce<NV, RED_SUM>(h, f, n, vec_ok, out);
}

extern "C" {

int mi355x_vec_set(mi355x_handle_t h, size_t n, double alpha, double *x) {
  return launch_map<0>(h, OpSet{alpha}, nullptr, nullptr, nullptr, x, n);
}
int mi355x_vec_copy(mi355x_handle_t h, size_t n, const double *x, double *y) {
  if (x == y) return 0;
  return launch_map<1>(h, OpCopy{}, x, nullptr, nullptr, y, n);
}
int mi355x_vec_scale(mi355x_handle_t h, size_t n, double alpha, double *x) {
  // VecScale_Seq (bvec1.c:183): alpha==0 -> set 0, alpha==1 -> nothing, else dscal
  if (alpha == 0.0) return mi355x_vec_set(h, n, 0.0, x);
  if (alpha == 1.0) return 0;
  return launch_map<1>(h, OpScale{alpha}, x, nullptr, nullptr, x, n);
}
int mi355x_vec_swap(mi355x_handle_t h, size_t n, double *x, double *y) {
  if (x == y || n == 0) return 0;
  hipLaunchKernelGGL(swap_kernel, dim3(mi355x_grid_for(n, 4)), dim3(MI355X_BLOCK), 0, h->stream, x, y, n);
  MI355X_LAUNCH_CHECK();
  return 0;
}
int mi355x_vec_axpy(mi355x_handle_t h, size_t n, double alpha, const double *x, double *y) {
  if (alpha == 0.0) return 0;  // bvec1.c:253
  return launch_map<2>(h, OpAxpy{alpha}, x, y, nullptr, y, n);
}
int mi355x_vec_aypx(mi355x_handle_t h, size_t n, double alpha, const double *x, double *y) {
  // dvec2.c:980-1009
  if (alpha == 0.0) return mi355x_vec_copy(h, n, x, y);
  if (alpha == 1.0) return mi355x_vec_axpy(h, n, 1.0, x, y);
  if (alpha == -1.0) return launch_map<2>(h, OpXmY{}, x, y, nullptr, y, n);
  return launch_map<2>(h, OpAypx{alpha}, x, y, nullptr, y, n);
}
int mi355x_vec_aypx_dev(mi355x_handle_t h, size_t n, const double *num_dev, double den, const double *x, double *y) {
  if (n == 0) return 0;
  return launch_tiles(h, n, all_aligned16(x, y), aypx_dev_kernel<true, false>, aypx_dev_kernel<false, false>, num_dev, den, x, y,
                      CGStepLen{0.0, 0.0, 0, nullptr}, (double *)nullptr);
}
int mi355x_vec_aypx_dev_x(mi355x_handle_t h, size_t n, const double *num_dev, double den, const double *x, double *y,
                          double beta, const double *dpi_dev, double dpiold, int check_sign, double *sol) {
  if (n == 0) return 0;
  return launch_tiles(h, n, all_aligned16(x, y, sol), aypx_dev_kernel<true, true>, aypx_dev_kernel<false, true>, num_dev, den, x, y,
                      CGStepLen{beta, dpiold, check_sign, dpi_dev}, sol);
}
int mi355x_vec_shift(mi355x_handle_t h, size_t n, double alpha, double *x) {
  return launch_map<1>(h, OpShift{alpha}, x, nullptr, nullptr, x, n);   // VecShift's loop (rvector.c): no special case for alpha == 0
}
int mi355x_vec_shift_dev(mi355x_handle_t h, size_t n, const double *num_dev, double den, double *x) {
  if (n == 0) return 0;
  return launch_tiles(h, n, all_aligned16(x), shift_dev_kernel<true>, shift_dev_kernel<false>, num_dev, den, x);
}
int mi355x_handle_publish_at(mi355x_handle_t h, const double *src_dev, int count, int dst_offset) {
  if (count < 0 || dst_offset < 0 || dst_offset + count > MI355X_SCRATCH_DOUBLES) return (int)hipErrorInvalidValue;
  const unsigned long long seq = ++h->seq;
  hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(MI355X_WAVE), 0, h->stream, src_dev, h->host_scratch + dst_offset, count,
                     const_cast<unsigned long long *>(h->host_seq), seq);
  MI355X_LAUNCH_CHECK();
  return 0;
}
int mi355x_handle_publish(mi355x_handle_t h, const double *src_dev, int count) { return mi355x_handle_publish_at(h, src_dev, count, 0); }
int mi355x_vec_axpby(mi355x_handle_t h, size_t n, double alpha, double beta, const double *x, double *y) {
  // bvec1.c:329-356
  if (alpha == 0.0) return mi355x_vec_scale(h, n, beta, y);
  if (beta == 1.0) return mi355x_vec_axpy(h, n, alpha, x, y);
  if (alpha == 1.0) return mi355x_vec_aypx(h, n, beta, x, y);
  if (beta == 0.0) return launch_map<1>(h, OpScale{alpha}, x, nullptr, nullptr, y, n);
  return launch_map<2>(h, OpAxpby{alpha, beta}, x, y, nullptr, y, n);
}
int mi355x_vec_waxpy(mi355x_handle_t h, size_t n, double alpha, const double *x, const double *y, double *w) {
  // dvec2.c:1094-1109
  if (alpha == 1.0) return launch_map<2>(h, OpXpY{}, x, y, nullptr, w, n);
  if (alpha == -1.0) return launch_map<2>(h, OpYmX{}, x, y, nullptr, w, n);
  if (alpha == 0.0) return mi355x_vec_copy(h, n, y, w);
  return launch_map<2>(h, OpAxpy{alpha}, x, y, nullptr, w, n);
}
int mi355x_vec_axpbypcz(mi355x_handle_t h, size_t n, double alpha, double beta, double gamma, const double *x,
                        const double *y, double *z) {
  if (alpha == 1.0) return launch_map<3>(h, OpAxpbypczA1{beta, gamma}, x, y, z, z, n);
  if (gamma == 1.0) return launch_map<3>(h, OpAxpbypczG1{alpha, beta}, x, y, z, z, n);
  if (gamma == 0.0) return launch_map<2>(h, OpAxpbypczG0{alpha, beta}, x, y, nullptr, z, n);
  return launch_map<3>(h, OpAxpbypcz{alpha, beta, gamma}, x, y, z, z, n);
}
int mi355x_vec_pointwise_mult(mi355x_handle_t h, size_t n, const double *x, const double *y, double *w) {
  return launch_map<2>(h, OpMul{}, x, y, nullptr, w, n);
}
int mi355x_vec_pointwise_divide(mi355x_handle_t h, size_t n, const double *x, const double *y, double *w) {
  return launch_map<2>(h, OpDiv{}, x, y, nullptr, w, n);
}
int mi355x_vec_reciprocal(mi355x_handle_t h, size_t n, double *x) {
  return launch_map<1>(h, OpRecip{}, x, nullptr, nullptr, x, n);
}
int mi355x_vec_jacobi_invert(mi355x_handle_t h, size_t n, double *d, int *nzero_dev) {
  if (nzero_dev) return (int)hipErrorInvalidValue;   // no count of the zero entries is kept (the header says so): refuse rather than leave it unwritten
  return launch_map<1>(h, OpJacInv{}, d, nullptr, nullptr, d, n);
}
int mi355x_stream_triad(mi355x_handle_t h, size_t n, double alpha, const double *b, const double *c, double *a) {
  return launch_map<2>(h, OpTriad{alpha}, b, c, nullptr, a, n);
}

int mi355x_vec_maxpy(mi355x_handle_t h, size_t n, int nv, const double *alpha, const double *const *y, double *x) {
  if (nv <= 0 || n == 0) return 0;
  return for_each_sweep(nv, [&](int pos, int g0, int ng4) {
    const int cnt = g0 + 4 * ng4;
    MaxpyArgs args = {};
    const int vec_ok = fill_basis(args.y, y + pos, cnt) && all_aligned16(x);
    for (int j = 0; j < cnt; ++j) args.a[j] = alpha[pos + j];
    args.nt = gs_streams(n, cnt);
    return with_groups(g0, ng4, [&](auto G0, auto NG4) {
      hipLaunchKernelGGL((maxpy_kernel<G0, NG4>), dim3(tile_grid<1>(n, vec_ok)), dim3(MI355X_BLOCK), 0, h->stream, args, x, n, vec_ok);
      MI355X_LAUNCH_CHECK();
      return 0;
    });
  });
}

int mi355x_vec_dot(mi355x_handle_t h, size_t n, const double *x, const double *y, double *out) {
  DotF f{x, y};
  f.nt = vec_streams(n);
  return launch_reduce<1, RED_SUM>(h, f, n, all_aligned16(x, y), out);
}
int mi355x_vec_sum(mi355x_handle_t h, size_t n, const double *x, double *out) {
  SumF f{x};
  f.nt = vec_streams(n);
  return launch_reduce<1, RED_SUM>(h, f, n, all_aligned16(x), out);
}
int mi355x_vec_max(mi355x_handle_t h, size_t n, const double *x, double *out) {
  return launch_reduce<2, RED_ARGMAX>(h, ExtremumF<RED_ARGMAX>{x}, n, all_aligned16(x), out);
}
int mi355x_vec_min(mi355x_handle_t h, size_t n, const double *x, double *out) {
  return launch_reduce<2, RED_ARGMIN>(h, ExtremumF<RED_ARGMIN>{x}, n, all_aligned16(x), out);
}
int mi355x_vec_norm(mi355x_handle_t h, size_t n, int type, const double *x, double *out) {
  const int v = all_aligned16(x);
  switch (type) {
    case 0: return launch_reduce<1, RED_SUM>(h, SumAbsF{x}, n, v, out);
    case 1:
    case 2: return launch_reduce<1, RED_SUM>(h, SumSqF{x, vec_streams(n)}, n, v, out);
    case 3: return launch_reduce<1, RED_MAX>(h, MaxAbsF{x}, n, v, out);
    case 4: return launch_reduce<2, RED_SUM>(h, Norm12F{x}, n, v, out);
    default: return (int)hipErrorInvalidValue;
  }
}
int mi355x_vec_dotnorm2(mi355x_handle_t h, size_t n, const double *s, const double *t, double *out) {
  DotNorm2F f{s, t};
  return launch_reduce<2, RED_SUM>(h, f, n, all_aligned16(s, t), out);
}
int mi355x_vec_cg_update(mi355x_handle_t h, size_t n, double a, const double *p, const double *w, const double *d,
                         double *x, double *r, double *z, double *out) {
  const CGUpdateF f{a, {p, w, d, x, r, z, vec_streams(n)}};
  return launch_reduce<3, RED_SUM>(h, f, n, all_aligned16(p, w, d, x, r, z), out);   // d == NULL (identity preconditioner) counts as aligned
}
int mi355x_vec_cg_update_dev(mi355x_handle_t h, size_t n, double beta, const double *dpi_dev, double dpiold, int check_sign,
                             const double *p, const double *w, const double *d, double *x, double *r, double *z, double *out,
                             int also_to_host) {
  const CGUpdateDevF f{{beta, dpiold, check_sign, dpi_dev}, {p, w, d, x, r, z, vec_streams(n)}};
  // d == NULL (identity preconditioner) and p, x == NULL (the x-less form) count as aligned
  return launch_reduce<4, RED_SUM>(h, f, n, all_aligned16(p, w, d, x, r, z), out, also_to_host != 0);
}
int mi355x_vec_cg_update_dev_nox(mi355x_handle_t h, size_t n, double beta, const double *dpi_dev, double dpiold, int check_sign,
                                 const double *w, const double *d, double *r, double *z, double *out, int also_to_host) {
  return mi355x_vec_cg_update_dev(h, n, beta, dpi_dev, dpiold, check_sign, nullptr, w, d, nullptr, r, z, out, also_to_host);
}
int mi355x_vec_pmult_dot(mi355x_handle_t h, size_t n, const double *x, const double *d, const double *y, double *w, double *out) {
  PMultDotF f{x, d, y, w};
  return launch_reduce<1, RED_SUM>(h, f, n, all_aligned16(x, d, y, w), out);
}
int mi355x_vec_pmult_dotnorm2(mi355x_handle_t h, size_t n, const double *x, const double *d, const double *s, double *w, double *out) {
  PMultDotNorm2F f{x, d, s, w};
  return launch_reduce<2, RED_SUM>(h, f, n, all_aligned16(x, d, s, w), out);
}
int mi355x_vec_bcgs_update(mi355x_handle_t h, size_t n, double alpha, double omega, const double *p, const double *s, const double *t,
                           const double *rp, double *x, double *r, double *out) {
  BcgsUpdateF f{alpha, omega, -omega, p, s, t, rp, x, r};
  return launch_reduce<2, RED_SUM>(h, f, n, all_aligned16(p, s, t, rp, x, r), out);
}

int mi355x_vec_cheby_step(mi355x_handle_t h, size_t n, double s, double a, double c, const double *w, const double *b, const double *d,
                          const double *pm, const double *pk, double *r, double *pn, int sums, double *out) {
  // b == NULL: w is the preconditioned residual as given (a general PC applied it): nothing to precondition, store or sum here
  if (!w || !pn || (!b && (d || r || sums)) || (sums && !out) || (a != 0.0 && !pm) || (c != 0.0 && !pk)) return (int)hipErrorInvalidValue;
  return launch_krylov_step(h, n, KrylovStepF{s, a, c, w, b, d, pm, pk, r, nullptr, pn, 0, 0}, sums, out);
}
int mi355x_vec_rich_step(mi355x_handle_t h, size_t n, double scale, const double *w, const double *b, const double *d, double *r, double *z, double *x) {
  if (!w || !b || !x) return (int)hipErrorInvalidValue;
  return launch_krylov_step(h, n, KrylovStepF{scale, 0.0, 0.0, w, b, d, nullptr, nullptr, r, z, x, 1, 0}, 0, nullptr);
}

int mi355x_vec_pipecg_step(mi355x_handle_t h, size_t n, int first, double ratio, double step, const double *nv, const double *mv, const double *d,
                           double *zrec, double *qrec, double *p, double *s, double *x, double *u, double *w, double *r, double *m_next,
                           int rides, double *out) {
  if (!nv || !mv || !zrec || !qrec || !p || !s || !x || !u || !w || !r || (out && (rides < 1 || rides > 3))) return (int)hipErrorInvalidValue;
  const PipeCGStepF f{ratio, step, nv, mv, d, zrec, qrec, p, s, x, u, w, r, m_next, first != 0, out ? rides : 0, vec_streams(n)};
  const int vec_ok = all_aligned16(nv, mv, d, zrec, qrec, p, s, x, u, w, r, m_next);   // d, m_next == NULL count as aligned
  if (out) return launch_reduce<2, RED_SUM>(h, f, n, vec_ok, out);                      // n == 0: zeros
  if (n == 0) return 0;
  return launch_tiles(h, n, vec_ok, pipecg_step_kernel, pipecg_step_kernel, f);
}

int mi355x_vec_minres_lanczos(mi355x_handle_t h, size_t n, double alpha, const double *alpha_dev, double beta, const double *d, double *r, double *z,
                              const double *v, const double *u, const double *vold, const double *uold, double *out) {
  if (!r || !z || !v || !u || !vold || !uold || !out) return (int)hipErrorInvalidValue;
  const MinresLanczosF f{alpha, beta, alpha_dev, d, v, u, vold, uold, r, z, vec_streams(n)};
  return launch_reduce<2, RED_SUM>(h, f, n, all_aligned16(d, r, z, v, u, vold, uold), out);   // d == NULL counts as aligned; n == 0: { 0, alpha }
}
int mi355x_vec_minres_update(mi355x_handle_t h, size_t n, int first, double rho2, double rho3, double irho1, double ceta, double ibeta,
                             const double *u, const double *w, double *wold, double *x, const double *r, const double *z, double *vnew, double *unew) {
  if (!r || !z || !vnew || !unew || (!first && (!u || !w || !wold || !x))) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (first) { u = w = nullptr; wold = x = nullptr; }                                        // not touched: their alignment does not count
  const MinresUpdateF f{rho2, rho3, irho1, ceta, ibeta, u, w, r, z, wold, x, vnew, unew, first != 0, vec_streams(n)};
  return launch_tiles(h, n, all_aligned16(u, w, wold, x, r, z, vnew, unew), minres_update_kernel, minres_update_kernel, f);
}

// a written vector of the three TFQMR / CGS sweeps that is another operand of the same call (NULL: an operand the form does not touch)
static inline bool written_is_operand(const double *const *written, int nw, const double *const *all, int na) {
  for (int i = 0; i < nw; ++i) {
    int seen = 0;
    for (int j = 0; j < na; ++j) seen += (written[i] != nullptr && all[j] == written[i]);
    if (seen > 1) return true;
  }
  return false;
}
int mi355x_vec_tfqmr_qt(mi355x_handle_t h, size_t n, double a, const double *u, const double *v, double *q, double *t, double *x) {
  if (!u || !v || !q || !t) return (int)hipErrorInvalidValue;
  const double *const written[] = {q, t, x}, *const all[] = {u, v, q, t, x};
  if (written_is_operand(written, 3, all, 5)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (a == 0.0) { v = nullptr; x = nullptr; }                                               // not touched: their alignment does not count
  const TfqmrQTF f{a, u, v, q, t, x, vec_streams(n)};
  return launch_tiles(h, n, all_aligned16(u, v, q, t, x), tfqmr_qt_kernel, tfqmr_qt_kernel, f);
}
int mi355x_vec_tfqmr_resid(mi355x_handle_t h, size_t n, double a, const double *auq, const double *rp, double *r, double *out) {
  if (!auq || !rp || !r || !out || auq == r || rp == r) return (int)hipErrorInvalidValue;
  if (a == 0.0) auq = nullptr;
  const TfqmrResidF f{-a, auq, rp, r, vec_streams(n)};
  return launch_reduce<2, RED_SUM>(h, f, n, all_aligned16(auq, rp, r), out);                 // n == 0: zeros
}
int mi355x_vec_tfqmr_update(mi355x_handle_t h, size_t n, int nhalves, double cf0, double eta0, double cf1, double eta1, int tail, double b,
                            double *d, double *x, double *u, double *q, const double *r, double *p) {
  if (nhalves < 0 || nhalves > 2) return (int)hipErrorInvalidValue;
  if (nhalves == 0) { d = nullptr; x = nullptr; }                                           // what this form does not touch is not looked at
  if (nhalves < 2 && !tail) q = nullptr;
  if (nhalves == 0 && !tail) u = nullptr;
  if (!tail) { r = nullptr; p = nullptr; }
  if ((nhalves >= 1 && (!d || !x || !u)) || (nhalves == 2 && !q) || (tail && (!u || !q || !r || !p))) return (int)hipErrorInvalidValue;
  const double *const written[] = {d, x, u, q, p}, *const all[] = {d, x, u, q, r, p};
  if (written_is_operand(written, 5, all, 6)) return (int)hipErrorInvalidValue;
  if (n == 0 || (nhalves == 0 && !tail)) return 0;
  const TfqmrUpdateF f{cf0, eta0, cf1, eta1, b, r, d, x, u, q, p, nhalves, tail != 0, vec_streams(n)};
  if (!((nhalves >= 1 && eta0 != 0.0) || (nhalves == 2 && eta1 != 0.0))) x = nullptr;       // alignment of what is neither loaded nor stored does not count
  if (tail && b == 0.0 && nhalves < 2) q = nullptr;
  return launch_tiles(h, n, all_aligned16(d, x, u, q, r, p), tfqmr_update_kernel, tfqmr_update_kernel, f);
}

int mi355x_vec_bicg_dirs(mi355x_handle_t h, size_t n, int first, double b, const double *zr, const double *zl, double *pr, double *pl) {
  if (!zr || !zl || !pr || !pl || pr == pl || pr == zr || pr == zl || pl == zr || pl == zl) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const BicgDirsF f{b, zr, zl, pr, pl, first != 0, vec_streams(n)};
  return launch_tiles(h, n, all_aligned16(zr, zl, pr, pl), bicg_dirs_kernel, bicg_dirs_kernel, f);
}
int mi355x_vec_bicg_update(mi355x_handle_t h, size_t n, double a, int pcmode, int which, const double *pr, const double *d, double *x,
                           double *rr, double *rl, double *zr, double *zl, double *out) {
  if (pcmode < 0 || pcmode > 2 || (which != 0 && which != 1) || !pr || !x || !rr || !rl || !zr || !zl || !out) return (int)hipErrorInvalidValue;
  if ((pcmode == 1) != (d != nullptr)) return (int)hipErrorInvalidValue;
  const double *const written[] = {x, rr, rl, zr, zl}, *const all[] = {x, rr, rl, zr, zl, pr, d};
  if (written_is_operand(written, 5, all, 7)) return (int)hipErrorInvalidValue;
  const BicgUpdateF f{a, pr, d, x, rr, rl, zr, zl, pcmode, which, vec_streams(n)};
  if (a == 0.0) { x = nullptr; pr = nullptr; if (!pcmode) { zr = nullptr; zl = nullptr; } }   // alignment of what is neither loaded nor stored does not count
  return launch_reduce<2, RED_SUM>(h, f, n, all_aligned16(pr, d, x, rr, rl, zr, zl), out);   // n == 0: zeros
}

int mi355x_vec_lsqr_bidiag(mi355x_handle_t h, size_t n, double coef, const double *coef2_dev, const double *x, double *y, double *out) {
  const bool needs_x = coef2_dev != nullptr || coef != 0.0;
  if (!y || !out || (needs_x && !x) || x == y) return (int)hipErrorInvalidValue;
  if (!needs_x) x = nullptr;                                                                  // not loaded: its alignment does not count
  const LsqrBidiagF f{coef, coef2_dev, x, y, vec_streams(n)};
  return launch_reduce<1, RED_SUM>(h, f, n, all_aligned16(x, y), out);                        // n == 0: { 0 }
}
int mi355x_vec_lsqr_update(mi355x_handle_t h, size_t n, double ialpha, double step, double cf, double irho2, int skip_w,
                           double *v1, double *x, double *w, double *se) {
  if (skip_w != 0 && skip_w != 1) return (int)hipErrorInvalidValue;
  const bool needs_v1 = !skip_w || ialpha != 1.0, needs_x = step != 0.0, needs_w = !skip_w || needs_x || se != nullptr;
  if ((needs_v1 && !v1) || (needs_x && !x) || (needs_w && !w)) return (int)hipErrorInvalidValue;
  if (!needs_v1) v1 = nullptr;                                                                // neither loaded nor stored: alignment and aliasing do not count
  if (!needs_x) x = nullptr;
  if (!needs_w) w = nullptr;
  const double *const vecs[] = {v1, x, w, se};
  if (written_is_operand(vecs, 4, vecs, 4)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const LsqrUpdateF f{ialpha, step, cf, irho2, v1, x, w, se, skip_w, vec_streams(n)};
  return launch_tiles(h, n, all_aligned16(v1, x, w, se), lsqr_update_kernel, lsqr_update_kernel, f);
}

// borthog2.c:63-64 + the norm of gmres.c:146: x += sum_j sign * coef_dev[j] * y_j, *out = sum x_new^2 (out: device or the
// handle's pinned scratch); coef_dev must not be written while this runs
int mi355x_vec_maxpy_dev_norm2(mi355x_handle_t h, size_t n, int nv, const double *coef_dev, double sign, const double *const *y,
                               double *x, double *out) {
  if (nv <= 0) return mi355x_vec_norm(h, n, 2, x, out);
  if (n == 0) return launch_reduce<1, RED_SUM>(h, SumSqF{x}, n, 1, out);
  return for_each_sweep(nv, [&](int pos, int g0, int ng4) {
    // an earlier sweep's sum is of no use: it goes to the last device scratch slot
    double *o = pos + g0 + 4 * ng4 == nv ? out : h->dev_scratch + (MI355X_SCRATCH_DOUBLES - 1);
    return with_groups(g0, ng4, [&](auto G0, auto NG4) {
      MaxpyNormF<G0, NG4> f;
      const int vec_ok = fill_basis(f.y, y + pos, f.NV) && all_aligned16(x);
      f.adev = coef_dev + pos; f.sign = sign; f.x = x;
      f.nt = gs_streams(n, f.NV);
      return launch_reduce<1, RED_SUM>(h, f, n, vec_ok, o);
    });
  });
}
int mi355x_vec_scale_rnorm_dev(mi355x_handle_t h, size_t n, const double *norm2_dev, double *x) {
  if (n == 0) return 0;
  const int vec_ok = all_aligned16(x);
  hipLaunchKernelGGL(scale_rnorm_dev_kernel, dim3(tile_grid<2>(n, vec_ok)), dim3(MI355X_BLOCK), 0, h->stream, norm2_dev, x, n, vec_ok);
  MI355X_LAUNCH_CHECK();
  return 0;
}
int mi355x_vec_scale_rnorm_dev_pmult(mi355x_handle_t h, size_t n, const double *norm2_dev, double *x, const double *d, double *z) {
  if (!norm2_dev || !x || !z || z == x || z == d || d == x) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const int vec_ok = all_aligned16(x, d, z);
  hipLaunchKernelGGL(scale_rnorm_dev_pmult_kernel, dim3(tile_grid<2>(n, vec_ok)), dim3(MI355X_BLOCK), 0, h->stream, norm2_dev, x, d, z, n, vec_ok);
  MI355X_LAUNCH_CHECK();
  return 0;
}
int mi355x_vec_mdot(mi355x_handle_t h, size_t n, int nv, const double *x, const double *const *y, double *out) {
  int pos = 0;
  static int width = 0;   // vectors per pass over x: MI355X_MDOT_WIDTH (16 or 32)
  if (!width) { const char *e = getenv("MI355X_MDOT_WIDTH"); width = (e && atoi(e) == 32) ? 32 : 16; }
  while (pos < nv) {
    int left = nv - pos;
    int cnt = left > width ? width : left;
    if (width == 16 && left > 16 && left < 24) cnt = (left + 1) / 2;   // two passes of similar width instead of 16 + a few
    int rc;
    switch (cnt) {
#define MDOT_CASE(N) case N: rc = launch_mdot<N>(h, n, x, y + pos, out + pos); break
      MDOT_CASE(1); MDOT_CASE(2); MDOT_CASE(3); MDOT_CASE(4); MDOT_CASE(5); MDOT_CASE(6); MDOT_CASE(7); MDOT_CASE(8);
      MDOT_CASE(9); MDOT_CASE(10); MDOT_CASE(11); MDOT_CASE(12); MDOT_CASE(13); MDOT_CASE(14); MDOT_CASE(15); MDOT_CASE(16);
      MDOT_CASE(17); MDOT_CASE(18); MDOT_CASE(19); MDOT_CASE(20); MDOT_CASE(21); MDOT_CASE(22); MDOT_CASE(23); MDOT_CASE(24);
      MDOT_CASE(25); MDOT_CASE(26); MDOT_CASE(27); MDOT_CASE(28); MDOT_CASE(29); MDOT_CASE(30); MDOT_CASE(31); MDOT_CASE(32);
#undef MDOT_CASE
      default: return (int)hipErrorInvalidValue;
    }
    if (rc) return rc;
    pos += cnt;
  }
  return 0;
}

}  // extern "C"
