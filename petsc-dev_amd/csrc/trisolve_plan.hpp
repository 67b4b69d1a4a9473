// Plan of a sync-free triangular solve: shared by the kernels + host analysis (trisolve.hip) and the device-side construction
// of the row plans (trisolve_build.hip).
#pragma once
#include "common.hpp"
#include <chrono>
#include <stdio.h>
#include <stdlib.h>

#define TRI_SENTINEL 0xFFF8DEADBEEFCAFEull
#define TRI_QUEUES 8
#define TRI_QSTRIDE 16          // queue counters 64 bytes apart
#define TRI_ALIGN_MIN 32        // by_level plans: levels of at least this many rows start on a slice boundary
#define TRI_SPIN_LIMIT (1 << 19)   // x ~1 us per poll once backed off: gives up after ~0.5 s
#define TRI_XCD_WORD (TRI_QUEUES * TRI_QSTRIDE)   // behind the queue counters: [0] the XCD that solves (0xffffffff: not chosen yet), [1] tickets


struct mi355x_trisolve_plan_s {
  int n, nslices, nchunks, upper;
  int *d_ptr;        // nslices + 1 entry offsets (multiples of 64)
  int *d_info;       // per position: (row length << 8) | sub-step inside the slice; padding positions: 0
  int *d_row;        // per position: the row it holds, -1 for padding
  int *d_col;        // sliced-ELL column POSITIONS
  double *d_val;     // sliced-ELL values
  double *d_dinv;    // upper: inverted diagonal per position
  double *d_rscale;  // upper, optional: factor applied to the right-hand side entry before the row's sum starts (ICC: D^-1 between the two solves)
  unsigned char *d_nsub;   // sub-steps per slice
  int *d_pos;        // per row: its position (for the other solve's gather of this solve's result)
  double *d_w;       // solution in position order, 64 * nslices doubles
  size_t nslots;     // doubles of d_w (node plans: nb per position)
  unsigned int *d_queue;   // TRI_QUEUES counters
  int *abort_flag;   // pinned + mapped
  int grid, sleep_cap;
  int by_level;      // rows in dependency-level order, levels on slice boundaries
  int nlev;
  int *levpos;       // host, 2 * nlev: first and one-past-last position of every dependency level (level-by-level fall-back)
  // node plans (nb > 1): a position holds a NODE -- up to nb consecutive rows with one shared column list (the inodes of the
  // reference, Mat_CheckInode); d_row = the node's first row, d_col = SLOTS (k * np + position) of the shared columns, d_val = nb
  // values per shared column, d_din = the couplings inside the node and (upper) the inverted diagonals, d_w = nb * np slots
  int nb, np;
  int spw;                 // node plans: slices (waves) per workgroup
  int split, maxcol;       // split-role kernel (loader + solver wavefront per workgroup): on, widest slice
  int one_xcd;             // split-role kernels: all participating workgroups on one XCD (hand-offs through its L2)
  int blkcols;             // the shared lists hold whole dependency nodes: one list entry per node, solution stored node by node
  unsigned char *d_nsz;    // per position: rows in the node
  double *d_din;           // [nb (nb - 1) / 2 + nb][np]
};

// every failure of a plan builder (`h`: the handle) leaves through these: pending copies out of the builder's local arrays are
// drained first, and the caller hands the half-built plan to mi355x_trisolve_plan_destroy
#define TRI_TRY(expr) do { const int e__ = (int)(expr); if (e__) { (void)hipStreamSynchronize(h->stream); return e__; } } while (0)
#define TRI_FAIL() do { (void)hipStreamSynchronize(h->stream); return (int)hipErrorInvalidValue; } while (0)

// MI355X_TRISOLVE_TIMING: where the set-up time of a plan goes (stderr), one line per step of a builder.  The device route's
// steps are asynchronous: its timer waits for `sync` before it reads the clock.
struct TriPlanTimer {
  bool on, upper, device;
  hipStream_t sync;
  double tlast;
  explicit TriPlanTimer(bool upper_, bool device_ = false, hipStream_t sync_ = nullptr)
      : on(getenv("MI355X_TRISOLVE_TIMING") != nullptr), upper(upper_), device(device_), sync(sync_), tlast(now()) {}
  static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  void tick(const char *what) {
    if (!on) return;
    if (device) (void)hipStreamSynchronize(sync);
    const double t = now();
    fprintf(stderr, "[mi355x trisolve plan %s%s] %-*s %.3f s\n", upper ? "U" : "L", device ? ", device" : "", device ? 22 : 28, what, t - tlast);
    tlast = t;
  }
};

// the part of a plan that does not depend on who laid out its arrays: the nslots solution slots armed with the sentinel, queue
// counters, abort flag, launch geometry with the defaults of the kernel family (trisolve.hip)
enum tri_family { TRI_ROWS, TRI_NODES };
int trisolve_plan_finish(mi355x_handle_t h, mi355x_trisolve_plan_s *p, size_t nslots, int nlev, tri_family family);
// construction of a row plan on the device from the host's factor arrays (trisolve_build.hip); same arrays as the host route's
int trisolve_plan_fill_device(mi355x_handle_t h, mi355x_trisolve_plan_s *p, int n, int nlev, const int *lev, const int *rp, const int *rl, const int *cj,
                              const double *cv, const double *dinv_host, const double *rscale_host, int by_level);
