// Coarsening for smoothed aggregation (PCGAMG, harness/gamg.c): a strength-of-connection mask over a square CSR matrix and an
// aggregation of its rows by a distance-2 maximal independent set.  Set-up kernels: one lane per row, rows in storage order.
//
// The contract (include/mi355x_kernels.h, DESIGN.md "PCGAMG") is integer and order-free:
//
//   strength   strong[t] = (j != i) && (fabs(a_t) > theta * sqrt(fabs(d_i) * fabs(d_j))) for the stored entry t = (i, j), in double,
//              in exactly that order; a comparison with a NaN on either side is false.
//   graph      undirected: i ~ j when the stored entry (i, j) OR the stored entry (j, i) is strong.  No transpose is built: a
//              propagation step pulls over a row's strong entries and pushes along them with a 64-bit atomicMax.  A maximum does not
//              depend on the order of its operands, so every array below has one possible content.
//   key        state << 62 | (mix(i) >> 2) << 32 | i, state 2 root, 1 undecided, 0 removed; mix the 32-bit finaliser below.
//   round      T = key; twice: every node takes the maximum of its T and its neighbours' T (from one buffer into another: a step
//              reaches distance 1, never further); an undecided node whose T is its own key becomes a root, an undecided node whose T
//              carries state 2 is removed.  The largest undecided key is always decided, so the loop ends; with fixed priorities the
//              roots are the greedy set of mi355x_coarsen_mis2_host (visit in decreasing key; root iff no root within distance 2).
//   aggregates a root's number is its rank among the roots in index order; a node with adjacent roots joins the one with the largest
//              key; any other node joins the root with the largest key among its neighbours' choices.
//
// No kernel waits on another workgroup.  The round loop is on the host: the undecided count lives in device memory and is read once
// per round (one host wait per round); the loop stops at MI355X_COARSEN_ROUND_CAP rounds with an error.  The roots are ranked by a host
// prefix sum over a downloaded flag array (one more host wait).
#include "common.hpp"
#include <algorithm>
#include <cmath>
#include <vector>

#define MI355X_COARSEN_ROUND_CAP 1024

typedef unsigned long long u64;

__host__ __device__ static inline unsigned int coarsen_mix(unsigned int h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
__host__ __device__ static inline u64 coarsen_key(unsigned int state, unsigned int i) {
  return ((u64)state << 62) | ((u64)(coarsen_mix(i) >> 2) << 32) | (u64)i;
}
#define KEY_STATE(k) ((unsigned int)((k) >> 62))
#define KEY_NODE(k) ((int)((k) & 0xffffffffull))

static inline unsigned coarsen_grid(int m) { return (unsigned)(((long)m + MI355X_BLOCK - 1) / MI355X_BLOCK); }

// a column outside [0, m) is never dereferenced: its entry is not strong
__global__ __launch_bounds__(MI355X_BLOCK) void strength_kernel(int m, const int *__restrict__ ai, const int *__restrict__ aj,
                                                               const double *__restrict__ aa, const double *__restrict__ diag, double theta,
                                                               unsigned char *__restrict__ strong) {
  const long i = (long)blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (i >= m) return;
  const double di = fabs(diag[i]);
  for (int t = ai[i]; t < ai[i + 1]; ++t) {
    const int j = aj[t];
    unsigned char s = 0;
    if (j != (int)i && (unsigned)j < (unsigned)m) s = fabs(aa[t]) > theta * __dsqrt_rn(di * fabs(diag[j])) ? 1 : 0;
    strong[t] = s;
  }
}

__global__ __launch_bounds__(MI355X_BLOCK) void mis2_init_kernel(int m, u64 *__restrict__ key) {
  const long i = (long)blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (i < m) key[i] = coarsen_key(1u, (unsigned int)i);
}

// dst (zero before the launch) = for every node the maximum of src over its closed neighbourhood.  only_zero: nodes whose src is
// nonzero keep out of it (the second aggregate pass: only a node without a choice asks its neighbours).
template <bool ONLY_ZERO>
__global__ __launch_bounds__(MI355X_BLOCK) void mis2_step_kernel(int m, const int *__restrict__ ai, const int *__restrict__ aj,
                                                                const unsigned char *__restrict__ strong, const u64 *__restrict__ src, u64 *dst) {
  const long i = (long)blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (i >= m) return;
  const u64 mine = src[i];
  u64 v = ONLY_ZERO ? 0ull : mine;
  for (int t = ai[i]; t < ai[i + 1]; ++t) {
    if (!strong[t]) continue;
    const int j = aj[t];
    if ((unsigned)j >= (unsigned)m) continue;
    const u64 theirs = src[j];
    if (!ONLY_ZERO || mine == 0ull) v = theirs > v ? theirs : v;            // pull
    if (mine != 0ull && (!ONLY_ZERO || theirs == 0ull)) atomicMax(&dst[j], mine);   // push
  }
  if (v != 0ull) atomicMax(&dst[i], v);
}

__global__ __launch_bounds__(MI355X_BLOCK) void mis2_decide_kernel(int m, u64 *__restrict__ key, const u64 *__restrict__ T, unsigned int *undecided) {
  const long i = (long)blockIdx.x * MI355X_BLOCK + threadIdx.x;
  int left = 0;
  if (i < m) {
    const u64 k = key[i];
    if (KEY_STATE(k) == 1u) {
      const u64 t = T[i];
      if (t == k) key[i] = coarsen_key(2u, (unsigned int)i);
      else if (KEY_STATE(t) == 2u) key[i] = coarsen_key(0u, (unsigned int)i);
      else left = 1;
    }
  }
  const u64 ballot = __ballot(left);
  if (ballot && (threadIdx.x % MI355X_WAVE) == (unsigned)(__ffsll((long long)ballot) - 1)) atomicAdd(undecided, (unsigned int)__popcll(ballot));
}

// the first aggregate pass: dst (zero before) = the largest root key in a node's closed neighbourhood, 0 when there is none
__global__ __launch_bounds__(MI355X_BLOCK) void mis2_adjacent_root_kernel(int m, const int *__restrict__ ai, const int *__restrict__ aj,
                                                                         const unsigned char *__restrict__ strong, const u64 *__restrict__ key, u64 *dst,
                                                                         int *__restrict__ isroot) {
  const long i = (long)blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (i >= m) return;
  const u64 mine = key[i];
  const bool root = KEY_STATE(mine) == 2u;
  isroot[i] = root ? 1 : 0;
  u64 v = root ? mine : 0ull;
  for (int t = ai[i]; t < ai[i + 1]; ++t) {
    if (!strong[t]) continue;
    const int j = aj[t];
    if ((unsigned)j >= (unsigned)m) continue;
    const u64 theirs = key[j];
    if (KEY_STATE(theirs) == 2u) v = theirs > v ? theirs : v;
    if (root) atomicMax(&dst[j], mine);
  }
  if (v != 0ull) atomicMax(&dst[i], v);
}

// agg[i] = rank of the root a node chose: its adjacent choice, else its neighbours' best
__global__ __launch_bounds__(MI355X_BLOCK) void mis2_number_kernel(int m, const u64 *__restrict__ c1, const u64 *__restrict__ c2,
                                                                  const int *__restrict__ rank, int *__restrict__ agg) {
  const long i = (long)blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (i >= m) return;
  const u64 c = c1[i] ? c1[i] : c2[i];
  agg[i] = rank[KEY_NODE(c)];            // (c == 0 cannot happen for a maximal set; node 0's rank is a number inside [0, nagg) anyway)
}

namespace {
// the undirected graph of the strong entries as adjacency lists (host twin only)
void strong_graph(int m, const int *ai, const int *aj, const unsigned char *strong, std::vector<int> &gi, std::vector<int> &gj) {
  gi.assign((size_t)m + 1, 0);
  for (int i = 0; i < m; ++i) for (int t = ai[i]; t < ai[i + 1]; ++t) {
    const int j = aj[t];
    if (strong[t] && j != i && (unsigned)j < (unsigned)m) { gi[(size_t)i + 1]++; gi[(size_t)j + 1]++; }
  }
  for (int i = 0; i < m; ++i) gi[(size_t)i + 1] += gi[(size_t)i];
  gj.assign((size_t)gi[(size_t)m], 0);
  std::vector<int> fill(gi.begin(), gi.end() - 1);
  for (int i = 0; i < m; ++i) for (int t = ai[i]; t < ai[i + 1]; ++t) {
    const int j = aj[t];
    if (strong[t] && j != i && (unsigned)j < (unsigned)m) { gj[(size_t)fill[(size_t)i]++] = j; gj[(size_t)fill[(size_t)j]++] = i; }
  }
}
}  // namespace

extern "C" {

int mi355x_csr_strength_host(int m, const int *ai, const int *aj, const double *aa, const double *diag, double theta, unsigned char *strong) {
  if (m < 0) return (int)hipErrorInvalidValue;
  if (m == 0) return 0;
  if (!ai || !diag || (ai[m] > 0 && (!aj || !aa || !strong))) return (int)hipErrorInvalidValue;
  for (int i = 0; i < m; ++i) {
    const double di = std::fabs(diag[i]);
    for (int t = ai[i]; t < ai[i + 1]; ++t) {
      const int j = aj[t];
      unsigned char s = 0;
      if (j != i && (unsigned)j < (unsigned)m) s = std::fabs(aa[t]) > theta * std::sqrt(di * std::fabs(diag[j])) ? 1 : 0;
      strong[t] = s;
    }
  }
  return 0;
}

int mi355x_csr_strength(mi355x_handle_t h, int m, const int *ai, const int *aj, const double *aa, const double *diag, double theta,
                        unsigned char *strong) {
  if (!h || m < 0) return (int)hipErrorInvalidValue;
  if (m == 0) return 0;
  if (!ai || !aj || !aa || !diag || !strong) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(strength_kernel, dim3(coarsen_grid(m)), dim3(MI355X_BLOCK), 0, h->stream, m, ai, aj, aa, diag, theta, strong);
  MI355X_LAUNCH_CHECK();
  return 0;
}

int mi355x_coarsen_round_cap(void) { return MI355X_COARSEN_ROUND_CAP; }

int mi355x_coarsen_mis2_host(int m, const int *ai, const int *aj, const unsigned char *strong, int *agg, int *nagg) {
  if (nagg) *nagg = 0;
  if (m < 0 || !nagg) return (int)hipErrorInvalidValue;
  if (m == 0) return 0;
  if (!ai || !agg || (ai[m] > 0 && (!aj || !strong))) return (int)hipErrorInvalidValue;
  return mi355x_guard([&]() -> int {
    std::vector<int> gi, gj;
    strong_graph(m, ai, aj, strong, gi, gj);
    std::vector<u64> key((size_t)m);
    std::vector<int> order((size_t)m);
    for (int i = 0; i < m; ++i) { key[(size_t)i] = coarsen_key(1u, (unsigned int)i); order[(size_t)i] = i; }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return key[(size_t)a] > key[(size_t)b]; });
    std::vector<unsigned char> root((size_t)m, 0), covered((size_t)m, 0);   // covered: a root lies within distance 2
    for (int u : order) {
      if (covered[(size_t)u]) continue;
      root[(size_t)u] = 1; covered[(size_t)u] = 1;
      for (int p = gi[(size_t)u]; p < gi[(size_t)u + 1]; ++p) {
        const int v = gj[(size_t)p];
        covered[(size_t)v] = 1;
        for (int q = gi[(size_t)v]; q < gi[(size_t)v + 1]; ++q) covered[(size_t)gj[(size_t)q]] = 1;
      }
    }
    std::vector<int> rank((size_t)m, 0);
    int n = 0;
    for (int i = 0; i < m; ++i) if (root[(size_t)i]) rank[(size_t)i] = n++;
    std::vector<u64> c1((size_t)m, 0);
    for (int i = 0; i < m; ++i) {
      u64 v = root[(size_t)i] ? coarsen_key(2u, (unsigned int)i) : 0ull;
      for (int p = gi[(size_t)i]; p < gi[(size_t)i + 1]; ++p) {
        const int j = gj[(size_t)p];
        if (root[(size_t)j]) v = std::max(v, coarsen_key(2u, (unsigned int)j));
      }
      c1[(size_t)i] = v;
    }
    for (int i = 0; i < m; ++i) {
      u64 c = c1[(size_t)i];
      if (!c) for (int p = gi[(size_t)i]; p < gi[(size_t)i + 1]; ++p) c = std::max(c, c1[(size_t)gj[(size_t)p]]);
      agg[i] = rank[(size_t)KEY_NODE(c)];
    }
    *nagg = n;
    return 0;
  });
}

int mi355x_coarsen_mis2(mi355x_handle_t h, int m, const int *ai, const int *aj, const unsigned char *strong, int *agg, int *nagg, int *rounds) {
  if (nagg) *nagg = 0;
  if (rounds) *rounds = 0;
  if (!h || m < 0 || !nagg) return (int)hipErrorInvalidValue;
  if (m == 0) return 0;
  if (!ai || !aj || !strong || !agg) return (int)hipErrorInvalidValue;
  return mi355x_guard([&]() -> int {
    // one allocation: key, two propagation buffers (u64 each), the root flags / ranks (int), the undecided count
    const size_t n8 = sizeof(u64) * (size_t)m, n4 = sizeof(int) * (size_t)m;
    char *work = nullptr;
    MI355X_TRY(hipMalloc((void **)&work, 3 * n8 + n4 + 16));
    struct Free { char *p; ~Free() { (void)hipFree(p); } } release{work};
    u64 *key = (u64 *)work, *Ta = (u64 *)(work + n8), *Tb = (u64 *)(work + 2 * n8);
    int *rank = (int *)(work + 3 * n8);
    unsigned int *count = (unsigned int *)(work + 3 * n8 + ((n4 + 7) & ~(size_t)7));
    const dim3 grid(coarsen_grid(m)), block(MI355X_BLOCK);
    hipStream_t st = h->stream;
    hipLaunchKernelGGL(mis2_init_kernel, grid, block, 0, st, m, key);
    MI355X_LAUNCH_CHECK();
    int r = 0;
    for (;;) {
      if (r >= MI355X_COARSEN_ROUND_CAP) return (int)hipErrorNotReady;
      unsigned int left = 0;
      MI355X_TRY(hipMemsetAsync(Ta, 0, 2 * n8, st));
      MI355X_TRY(hipMemsetAsync(count, 0, sizeof(unsigned int), st));
      hipLaunchKernelGGL(mis2_step_kernel<false>, grid, block, 0, st, m, ai, aj, strong, (const u64 *)key, Ta);
      hipLaunchKernelGGL(mis2_step_kernel<false>, grid, block, 0, st, m, ai, aj, strong, (const u64 *)Ta, Tb);
      hipLaunchKernelGGL(mis2_decide_kernel, grid, block, 0, st, m, key, (const u64 *)Tb, count);
      MI355X_LAUNCH_CHECK();
      MI355X_TRY(hipMemcpyAsync(&left, count, sizeof(left), hipMemcpyDeviceToHost, st));
      MI355X_TRY(hipStreamSynchronize(st));                    // the one host wait of a round
      ++r;
      if (!left) break;
    }
    if (rounds) *rounds = r;
    MI355X_TRY(hipMemsetAsync(Ta, 0, 2 * n8, st));
    hipLaunchKernelGGL(mis2_adjacent_root_kernel, grid, block, 0, st, m, ai, aj, strong, (const u64 *)key, Ta, rank);
    hipLaunchKernelGGL(mis2_step_kernel<true>, grid, block, 0, st, m, ai, aj, strong, (const u64 *)Ta, Tb);
    MI355X_LAUNCH_CHECK();
    std::vector<int> flags((size_t)m);
    MI355X_TRY(hipMemcpyAsync(flags.data(), rank, n4, hipMemcpyDeviceToHost, st));
    MI355X_TRY(hipStreamSynchronize(st));
    int n = 0;
    for (int i = 0; i < m; ++i) { const int f = flags[(size_t)i]; flags[(size_t)i] = n; n += f; }
    MI355X_TRY(hipMemcpyAsync(rank, flags.data(), n4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(mis2_number_kernel, grid, block, 0, st, m, (const u64 *)Ta, (const u64 *)Tb, (const int *)rank, agg);
    MI355X_LAUNCH_CHECK();
    MI355X_TRY(hipStreamSynchronize(st));                      // (flags and the workspace go away here)
    *nagg = n;
    return 0;
  });
}

}  // extern "C"
