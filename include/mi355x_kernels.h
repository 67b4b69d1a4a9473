/*
 * mi355x_kernels.h -- C ABI of the MI355X (gfx950 / CDNA4) kernel library
 * (libmi355x_kernels.so) behind the PETSc HIPMI355X Vec/Mat implementations.
 *
 * Plain C: raw device pointers, sizes, an opaque handle that owns one HIP
 * stream.  No PETSc types, no torch types.  Every function returns 0 on
 * success or a non-zero hipError_t value (mi355x_error_string() decodes it);
 * nothing throws, nothing exits.  PetscScalar = double, PetscInt = int32
 * (reference: include/petscsys.h:188, include/petscmath.h:198).
 *
 * Each entry cites the reference CPU routine it replaces (path relative to
 * the PETSc tree, erdc/petsc-dev 3.3.0-dev).  Floating-point contract: all
 * kernels are compiled with -ffp-contract=off, i.e. a*b+c is a rounded
 * multiply followed by a rounded add, exactly what the reference's C loops
 * do when built without FMA.  Element-wise kernels and the row-sequential
 * SpMV paths therefore reproduce the reference bit for bit; reductions use
 * a fixed tree (run-to-run reproducible) and agree to a stated tolerance.
 */
#ifndef MI355X_KERNELS_H
#define MI355X_KERNELS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355x_handle_s    *mi355x_handle_t;    /* one HIP stream + reduction workspace */
typedef struct mi355x_event_s     *mi355x_event_t;     /* hipEvent_t */
typedef struct mi355x_spmv_plan_s *mi355x_spmv_plan_t; /* row-block partition of one CSR matrix */

/* ---- runtime --------------------------------------------------------- */
const char *mi355x_error_string(int err);
int  mi355x_device_count(int *count);
int  mi355x_set_device(int dev);
int  mi355x_get_device(int *dev);
int  mi355x_device_name(char *buf, size_t len);
int  mi355x_device_synchronize(void);
int  mi355x_mem_info(size_t *free_bytes, size_t *total_bytes);   /* hipMemGetInfo of the current device */
/* host threads THIS process may use for the set-up passes (pattern analyses, factorisation, plan construction), at most cap:
 * the CPUs of its affinity mask, cut to the cgroup's CPU quota, shared among the ranks torchrun started on this node
 * (LOCAL_WORLD_SIZE).  MI355X_HOST_THREADS=<n> in the environment overrides the count, cap included, up to 64.  Never less than 1. */
int  mi355x_host_threads(int cap);
/* fn(ctx, lo, hi) over [0, n) in nth contiguous chunks (lo = n k / nth, hi = n (k + 1) / nth, k = 0 .. nth - 1), chunk 0 on the
 * calling thread, the others on host threads of their own (on the caller, after the others, where a thread cannot be started).
 * Returns after every chunk has run: 0, or the first nonzero status a chunk returned. */
int  mi355x_host_parallel_ranges(long n, int nth, int (*fn)(void *ctx, long lo, long hi), void *ctx);

int  mi355x_handle_create(mi355x_handle_t *h);
int  mi355x_handle_destroy(mi355x_handle_t h);
int  mi355x_handle_synchronize(mi355x_handle_t h);
/* wait for the last reduction written to the handle's pinned scratch (polls a completion word the kernel stores
 * after the result; bounded, falls back to a stream synchronise) */
int  mi355x_handle_wait_result(mi355x_handle_t h);
/* queue a copy of count (<= 64) doubles from device memory to the pinned scratch followed by the completion number:
 * mi355x_handle_wait_result then returns as soon as THAT point of the stream is reached, whatever was queued behind it */
int  mi355x_handle_publish(mi355x_handle_t h, const double *src_dev, int count);
int  mi355x_handle_publish_at(mi355x_handle_t h, const double *src_dev, int count, int dst_offset);   /* into host_scratch[dst_offset ..) */
void *mi355x_handle_stream(mi355x_handle_t h);           /* the raw hipStream_t */
/* pinned, device-visible scratch of >= 64 doubles owned by the handle
 * (reduction results are written here by the device, read by the host
 * after mi355x_handle_synchronize) */
double *mi355x_handle_host_scratch(mi355x_handle_t h);
double *mi355x_handle_device_scratch(mi355x_handle_t h);  /* >= 64 doubles in HBM */

int  mi355x_malloc(void **dptr, size_t bytes);
int  mi355x_free(void *dptr);
int  mi355x_host_malloc(void **hptr, size_t bytes);      /* pinned + device-mapped */
int  mi355x_host_free(void *hptr);
int  mi355x_memcpy_h2d(mi355x_handle_t h, void *dst, const void *src, size_t bytes); /* async on h */
int  mi355x_memcpy_d2h(mi355x_handle_t h, void *dst, const void *src, size_t bytes); /* async on h */
int  mi355x_memcpy_d2d(mi355x_handle_t h, void *dst, const void *src, size_t bytes); /* async on h */
int  mi355x_memset(mi355x_handle_t h, void *dst, int byte, size_t bytes);

int  mi355x_event_create(mi355x_event_t *e);
int  mi355x_event_destroy(mi355x_event_t e);
int  mi355x_event_record(mi355x_event_t e, mi355x_handle_t h);
int  mi355x_event_synchronize(mi355x_event_t e);
int  mi355x_event_elapsed_ms(mi355x_event_t start, mi355x_event_t stop, float *ms);
int  mi355x_handle_wait_event(mi355x_handle_t h, mi355x_event_t e);  /* hipStreamWaitEvent */

/* hipGraph capture of whatever is enqueued on the handle between begin and end; replay with one call */
int  mi355x_graph_capture_begin(mi355x_handle_t h);
int  mi355x_graph_capture_end(mi355x_handle_t h, void **graph_exec);
int  mi355x_graph_launch(mi355x_handle_t h, void *graph_exec);
int  mi355x_graph_destroy(void *graph_exec);

/* ---- Vec element-wise kernels (24-32 B/element, HBM-bound) ------------ */
/* VecSet_Seq          src/vec/vec/impls/seq/dvec2.c:722      x[i] = alpha */
int mi355x_vec_set(mi355x_handle_t h, size_t n, double alpha, double *x);
/* VecCopy_Seq         src/vec/vec/impls/seq/bvec2.c:464      y = x */
int mi355x_vec_copy(mi355x_handle_t h, size_t n, const double *x, double *y);
/* VecScale_Seq        src/vec/vec/impls/seq/bvec1.c:183      x *= alpha (dscal) */
int mi355x_vec_scale(mi355x_handle_t h, size_t n, double alpha, double *x);
/* VecSwap_Seq         src/vec/vec/impls/seq/bvec2.c:519 */
int mi355x_vec_swap(mi355x_handle_t h, size_t n, double *x, double *y);
/* VecAXPY_Seq         src/vec/vec/impls/seq/bvec1.c:244      y += alpha x (daxpy) */
int mi355x_vec_axpy(mi355x_handle_t h, size_t n, double alpha, const double *x, double *y);
/* VecAYPX_Seq         src/vec/vec/impls/seq/dvec2.c:971      y = x + alpha y */
int mi355x_vec_aypx(mi355x_handle_t h, size_t n, double alpha, const double *x, double *y);
/* VecAXPBY_Seq        src/vec/vec/impls/seq/bvec1.c:320      y = alpha x + beta y */
int mi355x_vec_axpby(mi355x_handle_t h, size_t n, double alpha, double beta, const double *x, double *y);
/* VecWAXPY_Seq        src/vec/vec/impls/seq/dvec2.c:1082     w = y + alpha x */
int mi355x_vec_waxpy(mi355x_handle_t h, size_t n, double alpha, const double *x, const double *y, double *w);
/* VecAXPBYPCZ_Seq     src/vec/vec/impls/seq/bvec1.c:418      z = alpha x + beta y + gamma z */
int mi355x_vec_axpbypcz(mi355x_handle_t h, size_t n, double alpha, double beta, double gamma,
                        const double *x, const double *y, double *z);
/* VecPointwiseMult_Seq   src/vec/vec/impls/seq/bvec2.c:234   w = x .* y (w may alias x or y) */
int mi355x_vec_pointwise_mult(mi355x_handle_t h, size_t n, const double *x, const double *y, double *w);
/* VecPointwiseDivide_Seq src/vec/vec/impls/seq/bvec2.c:298   w = x ./ y */
int mi355x_vec_pointwise_divide(mi355x_handle_t h, size_t n, const double *x, const double *y, double *w);
/* VecReciprocal_Default  src/vec/vec/utils/vinv.c            x[i] = 1/x[i] where x[i] != 0 */
int mi355x_vec_reciprocal(mi355x_handle_t h, size_t n, double *x);
/* PCSetUp_Jacobi host loop  src/ksp/pc/impls/jacobi/jacobi.c:182-190  d = (d==0) ? 1 : 1/d, done on device (-0.0 counts as zero;
 * 1/inf = 0).  The zero entries are not counted (the reference only uses the count for a PetscInfo line): nzero_dev must be NULL,
 * anything else returns hipErrorInvalidValue and leaves d alone. */
int mi355x_vec_jacobi_invert(mi355x_handle_t h, size_t n, double *d, int *nzero_dev);
/* VecMAXPY_Seq        src/vec/vec/impls/seq/dvec2.c:836      x += sum_j alpha[j] y_j ; grouping
 * (nv%4 first, then fours) and left-to-right product sums follow petscaxpy.h:101-110.
 * y: host array of nv device pointers; alpha: host array. */
int mi355x_vec_maxpy(mi355x_handle_t h, size_t n, int nv, const double *alpha, const double *const *y, double *x);

/* ---- Vec reductions (8-16 B/element) ---------------------------------- */
/* Results are written to `out` (device-accessible: HBM or pinned host memory) when the
 * kernel completes on the handle's stream; the caller synchronises.  Two-level
 * fixed-shape tree: per-lane strided partial -> wavefront shuffle -> LDS -> per-block
 * partial -> last-arriving block sums the per-block partials in block order. */
/* VecDot_Seq/VecTDot_Seq  src/vec/vec/impls/seq/bvec1.c:57,122   out[0] = sum x_i y_i */
int mi355x_vec_dot(mi355x_handle_t h, size_t n, const double *x, const double *y, double *out);
/* VecNorm_Seq         src/vec/vec/impls/seq/bvec2.c:605
 * type 0: NORM_1 -> out[0]=sum|x|; 1: NORM_2 -> out[0]=sum x^2 (caller takes sqrt, as pvec2.c:62 does);
 * 3: NORM_INFINITY -> out[0]=max|x| (NaN propagates, bvec2.c:628-630); 4: NORM_1_AND_2 -> out[0]=sum|x|, out[1]=sum x^2 */
int mi355x_vec_norm(mi355x_handle_t h, size_t n, int type, const double *x, double *out);
/* VecDotNorm2 (BiCGStab)  src/vec/vec/utils/vinv.c:1200   out[0] = sum s_i t_i, out[1] = sum t_i^2 */
int mi355x_vec_dotnorm2(mi355x_handle_t h, size_t n, const double *s, const double *t, double *out);
/* VecAYPX with the scalar's numerator on the device: y = x + (*num_dev / den) y (alpha == 0 -> copy, dvec2.c:980).
 * KSPSolve_CG's p = z + (beta_new/beta_old) p when beta_new has not reached the host yet. */
int mi355x_vec_aypx_dev(mi355x_handle_t h, size_t n, const double *num_dev, double den, const double *x, double *y);
/* Fused CG update, one sweep for cg.c:206-232 + PCApply_Jacobi (jacobi.c:266-277):
 * x += a p; r += (-a) w; z = r .* d (d == NULL: z = r); out[0] = sum z*z, out[1] = sum z*r, out[2] = sum r*r.  Same
 * bits as mi355x_vec_axpy x2, mi355x_vec_pointwise_mult, mi355x_vec_norm(2) of z / of r, mi355x_vec_dot in sequence: for
 * a == 0 (either sign) x and r are left alone as VecAXPY leaves them (bvec1.c:253); z and the sums are still produced. */
int mi355x_vec_cg_update(mi355x_handle_t h, size_t n, double a, const double *p, const double *w, const double *d,
                         double *x, double *r, double *z, double *out);
/* The same sweep with the step length formed on the device: a = beta / *dpi_dev (dpi = p'w left in device memory by
 * mi355x_vec_dot, all-reduced there on several ranks).  The break-down tests of cg.c:196-199 (dpi NaN/Inf, dpi == 0,
 * check_sign && dpi*dpiold <= 0) are evaluated in the kernel: if one fires, x, r, z are left untouched.
 * out[0] = sum z*z, out[1] = sum z*r, out[2] = sum r*r, out[3] = dpi (for the host's own copy of those tests; it is summed
 * with the +0.0 of every other lane, so a dpi of -0.0 arrives as +0.0).
 * also_to_host != 0 with a device `out`: the four values are stored to the first pinned scratch slots as well, followed by the completion
 * number (mi355x_handle_wait_result) -- the result serves a later kernel and the host without a second launch. */
int mi355x_vec_cg_update_dev(mi355x_handle_t h, size_t n, double beta, const double *dpi_dev, double dpiold, int check_sign,
                             const double *p, const double *w, const double *d, double *x, double *r, double *z, double *out,
                             int also_to_host);
/* The same sweep without x += a p (the AYPX that reads p next does it: mi355x_vec_aypx_dev_x): reads r, w, d, writes r, z
 * -- 5 vector passes instead of 8.  Same a, same break-down tests, same r, z and out[0..3] bits. */
int mi355x_vec_cg_update_dev_nox(mi355x_handle_t h, size_t n, double beta, const double *dpi_dev, double dpiold, int check_sign,
                                 const double *w, const double *d, double *r, double *z, double *out, int also_to_host);
/* mi355x_vec_aypx_dev that first applies the CG step the x-less update left out, with the y it is about to overwrite:
 * a = beta / *dpi_dev with the tests of mi355x_vec_cg_update_dev; a != 0: sol = sol + a y; then y = x + (*num_dev / den) y.
 * Bits of mi355x_vec_cg_update_dev's x followed by mi355x_vec_aypx_dev's y. */
int mi355x_vec_aypx_dev_x(mi355x_handle_t h, size_t n, const double *num_dev, double den, const double *x, double *y,
                          double beta, const double *dpi_dev, double dpiold, int check_sign, double *sol);
/* Fused forms for KSPSolve_BCGS (src/ksp/ksp/impls/bcgs/bcgs.c:43-160); same bits as the calls they replace.
 * pmult_dot:      w = x .* d (PCApply_Jacobi jacobi.c:266; d == NULL: identity), out[0] = sum w*y       (bcgs.c:108-109)
 * pmult_dotnorm2: w = x .* d,                       out[0] = sum s*w, out[1] = sum w*w               (bcgs.c:116-117)
 * bcgs_update:    x = alpha p + omega s + x ; r = s - omega t ; out[0] = sum r*r, out[1] = sum r*rp  (bcgs.c:134-136,103) */
int mi355x_vec_pmult_dot(mi355x_handle_t h, size_t n, const double *x, const double *d, const double *y, double *w, double *out);
int mi355x_vec_pmult_dotnorm2(mi355x_handle_t h, size_t n, const double *x, const double *d, const double *s, double *w, double *out);
int mi355x_vec_bcgs_update(mi355x_handle_t h, size_t n, double alpha, double omega, const double *p, const double *s, const double *t,
                           const double *rp, double *x, double *r, double *out);
/* One step of KSPSolve_Chebychev (src/ksp/ksp/impls/cheby/cheby.c) / KSPSolve_Richardson (src/ksp/ksp/impls/rich/rich.c) behind
 * the product w = A p: the residual, a diagonal preconditioner and the update in one sweep, same bits as mi355x_vec_aypx(-1),
 * mi355x_vec_pointwise_mult, mi355x_vec_scale and mi355x_vec_axpy (x2) in sequence.
 * cheby_step:  rv = b - w ; r != NULL: r = rv (r may be w) ; zv = d ? rv * d : rv ;
 *              t = s == 1 ? zv : (s == 0 ? +0.0 : s * zv) ; a != 0: t = t + a * pm ; c != 0: t = t + c * pk ; pn = t
 *              sums != 0: out[0] = sum zv*zv, out[1] = sum rv*rv (the trees of mi355x_vec_norm(type 1) over z and r for an aligned
 *              view; out: device or the handle's pinned scratch) ; sums == 0: out is not touched, nothing is reduced.
 *              b == NULL: w already is the preconditioned residual (zv = w; d, r must be NULL, sums 0), and then w may be pn.
 * rich_step:   rv = b - w ; r != NULL: r = rv (r may be w) ; zv = d ? rv * d : rv ; z != NULL: z = zv ; scale != 0: x = x + scale * zv
 * pn overlaps no input (but for w with b == NULL); an operand a form does not read (pm for a == 0, pk for c == 0) may be NULL;
 * n == 0 launches nothing and, with sums, leaves zeros in out. */
int mi355x_vec_cheby_step(mi355x_handle_t h, size_t n, double s, double a, double c, const double *w, const double *b, const double *d,
                          const double *pm, const double *pk, double *r, double *pn, int sums, double *out);
int mi355x_vec_rich_step(mi355x_handle_t h, size_t n, double scale, const double *w, const double *b, const double *d, double *r, double *z, double *x);
/* The body of KSPSolve_PIPECG's loop (src/ksp/ksp/impls/cg/pipecg/pipecg.c:138-175) behind m = B w (mv) and n = A m (nv), one sweep with
 * the bits of mi355x_vec_copy / _aypx (x4), mi355x_vec_axpy (x4), mi355x_vec_pointwise_mult and mi355x_vec_dot / _norm(type 1) in sequence:
 *   first != 0: zrec = nv ; qrec = mv ; p = u ; s = w (the old contents are not read)
 *   otherwise:  zrec = nv + ratio zrec ; qrec = mv + ratio qrec ; p = u + ratio p ; s = w + ratio s  (mi355x_vec_aypx's cases 0, 1, -1)
 *   step != 0:  x = x + step p ; u = u + (-step) qrec ; w = w + (-step) zrec ; r = r + (-step) s  (step == 0: none of the four is written)
 *   m_next != NULL: m_next = w .* d (d == NULL: a copy of w); m_next may be mv, every load of an element precedes its stores
 *   out != NULL: out[0] = sum w*u, out[1] = sum r*r (rides 1), sum u*u (rides 2) or sum r*u (rides 3) over the updated vectors (for an
 *   aligned view the trees of mi355x_vec_dot / mi355x_vec_norm(type 1); out: device or the handle's pinned scratch); n == 0: zeros.
 *   out == NULL: the pure element-wise form, nothing reduced.
 * An operand a special case skips is not loaded.  A missing vector, or rides outside 1..3 with out: nonzero, nothing touched. */
int mi355x_vec_pipecg_step(mi355x_handle_t h, size_t n, int first, double ratio, double step, const double *nv, const double *mv, const double *d,
                           double *zrec, double *qrec, double *p, double *s, double *x, double *u, double *w, double *r, double *m_next,
                           int rides, double *out);
/* The two sweeps of an iteration of KSPSolve_MINRES (src/ksp/ksp/impls/minres/minres.c) behind r = A u and alpha = u'r, with the bits of
 * mi355x_vec_pointwise_mult, mi355x_vec_axpy, mi355x_vec_copy, mi355x_vec_scale and mi355x_vec_dot run one call at a time.
 * lanczos:  d != NULL: z = r .* d (PCApply_Jacobi, z not read); d == NULL: z as given;
 *           r = r + (-alpha) v ; z = z + (-alpha) u ; r = r + (-beta) vold ; z = z + (-beta) uold   (in this order; alpha == 0 / beta == 0:
 *           that pair untouched and v, u / vold, uold not loaded);  out[0] = sum r*z over the updated vectors (for an aligned view the tree
 *           of mi355x_vec_dot), out[1] = alpha;  out: device or the handle's pinned scratch;  n == 0: { 0, alpha }.
 *           alpha_dev != NULL: alpha is read from device memory (what mi355x_vec_dot left there) and the host argument is ignored.
 * update:   wn = u ; wn = wn + (-rho2) w ; wn = wn + (-rho3) wold ; wn = irho1 wn, stored over wold ; x = x + ceta wn ;
 *           vnew = ibeta r ; unew = ibeta z.   rho2 / rho3 / ceta == 0: that AXPY skipped, its operand not loaded (ceta == 0: x untouched);
 *           irho1, ibeta: mi355x_vec_scale's cases (0: zeros, nothing loaded; 1: a copy).  first != 0 (the solve start): vnew and unew
 *           alone, nothing else read or written (u, w, wold, x may be NULL).  A pure map: nothing reduced.
 * No written vector is another operand of the same call (wold is read and written in place).  A missing vector: nonzero, nothing touched. */
int mi355x_vec_minres_lanczos(mi355x_handle_t h, size_t n, double alpha, const double *alpha_dev, double beta, const double *d, double *r, double *z,
                              const double *v, const double *u, const double *vold, const double *uold, double *out);
int mi355x_vec_minres_update(mi355x_handle_t h, size_t n, int first, double rho2, double rho3, double irho1, double ceta, double ibeta,
                             const double *u, const double *w, double *wold, double *x, const double *r, const double *z, double *vnew, double *unew);
/* The three sweeps of an iteration of KSPSolve_TFQMR (src/ksp/ksp/impls/tfqmr/tfqmr.c) and KSPSolve_CGS (src/ksp/ksp/impls/cgs/cgs.c) around
 * the two applications of the preconditioned operator, with the bits of mi355x_vec_waxpy, mi355x_vec_axpy, mi355x_vec_aypx,
 * mi355x_vec_norm(type 1) and mi355x_vec_dot run one call at a time, their scalar special cases (0, 1, -1) included; an operand a special
 * case skips is not loaded, a vector no case changes is not stored.
 * qt:      q = u + (-a) v ; t = q + u ; x != NULL (CGS): x = x + a t.   a == 0: q = u, v not loaded, x untouched.  A pure map.
 * resid:   r = r + (-a) auq ; out = { sum r*r , sum r*rp } over the updated r (for an aligned view the trees of mi355x_vec_norm(type 1)
 *          and mi355x_vec_dot);  a == 0: r untouched, auq not loaded;  out: device or the handle's pinned scratch;  n == 0: { 0, 0 }.
 * update:  nhalves >= 1: d = u + cf0 d ; x = x + eta0 d.   nhalves == 2: then d = q + cf1 d ; x = x + eta1 d (the halves read the OLD u
 *          and q).   tail != 0: un = r + b q ; qn = q + b p ; pn = un + b qn, stored to u, q, p.   nhalves == 0 (CGS): d and x not
 *          touched and may be NULL; tail == 0: u, q, p, r not touched by the tail (r, p may be NULL; q too when nhalves < 2; u too when
 *          nhalves == 0).  A pure map: nothing reduced.
 * Nonzero and nothing touched: a vector the form touches is missing, nhalves is not 0, 1 or 2, or a written vector (q, t, x; r; d, x, u,
 * q, p) is another operand of the same call. */
int mi355x_vec_tfqmr_qt(mi355x_handle_t h, size_t n, double a, const double *u, const double *v, double *q, double *t, double *x);
int mi355x_vec_tfqmr_resid(mi355x_handle_t h, size_t n, double a, const double *auq, const double *rp, double *r, double *out);
int mi355x_vec_tfqmr_update(mi355x_handle_t h, size_t n, int nhalves, double cf0, double eta0, double cf1, double eta1, int tail, double b,
                            double *d, double *x, double *u, double *q, const double *r, double *p);
/* The two sweeps of an iteration of KSPSolve_BiCG (src/ksp/ksp/impls/bicg/bicg.c), every output with the bits of the separate calls.
 *   _dirs    first: pr = zr, pl = zl (VecCopy x2); else pr = zr + b pr, pl = zl + b pl (VecAYPX x2 with its special cases).  Nothing is
 *            reduced.  No two of the four may be the same array (hipErrorInvalidValue, nothing written).
 *   _update  x += a pr ; rr -= a zr ; rl -= a zl (VecAXPY x3; a == 0: nothing moved).  pcmode 1: zr = rr .* d, zl = rl .* d (PCJACOBI both
 *            ways); pcmode 2: zr = rr, zl = rl (PCNONE); pcmode 0: zr and zl are only read.  out[0] = sum zr*rl (VecDot(Zr, Rl)), out[1] =
 *            sum zr*zr (which == 0) or sum rr*rr (which == 1), the sum VecNorm takes the root of, over the updated vectors in the
 *            fixed-tree order of mi355x_vec_dot / _norm; pcmode 0: out = { 0, sum rr*rr }.  out: device memory or the handle's pinned
 *            scratch.  hipErrorInvalidValue and nothing written for a NULL operand, d given without pcmode 1 or missing with it, pcmode
 *            or which out of range, or a written vector that is another operand. */
int mi355x_vec_bicg_dirs(mi355x_handle_t h, size_t n, int first, double b, const double *zr, const double *zl, double *pr, double *pl);
int mi355x_vec_bicg_update(mi355x_handle_t h, size_t n, double a, int pcmode, int which, const double *pr, const double *d, double *x,
                           double *rr, double *rl, double *zr, double *zl, double *out);
/* The two sweeps of an iteration of KSPSolve_LSQR (src/ksp/ksp/impls/lsqr/lsqr.c) around u1 = A v and v1 = A^T u1, with the bits of
 * mi355x_vec_axpy, mi355x_vec_norm(type 2), mi355x_vec_scale, mi355x_vec_copy, mi355x_vec_pointwise_mult and mi355x_vec_aypx run one call at
 * a time.
 * bidiag:  y = y + (-coef) x ; out[0] = sum y*y over the updated y (for an aligned view the tree of mi355x_vec_norm(type 2): the square,
 *          the caller roots it); out: device or the handle's pinned scratch; n == 0: { 0 }.  coef == 0: y untouched, x not loaded (may be
 *          NULL).  coef2_dev != NULL: coef = sqrt(*coef2_dev) is formed on the device -- the sum an earlier call of this function left in
 *          device memory, rooted as the host roots it -- and the host argument is ignored.
 * update:  v1 = ialpha v1 (mi355x_vec_scale's cases: 1: v1 not stored; 0: zeros, v1 not loaded) ; x = x + step w (step == 0: x untouched,
 *          may be NULL) ; se != NULL: se = se + irho2 (w .* w) (the four calls copy, square, scale, AXPY) ; w = v1 + cf w over the scaled v1
 *          (mi355x_vec_aypx's cases 0, 1, -1).  skip_w == 1: w is not stored (LSQR's breakdown exit: x and se still take the old w; with
 *          ialpha == 1 v1 may be NULL; with step == 0 and se == NULL as well w may be NULL and the call is a plain scaling of v1).  A pure
 *          map: nothing reduced.
 * hipErrorInvalidValue and nothing touched for an operand the form needs that is NULL, skip_w outside {0, 1}, or a written vector that is
 * another operand of the same call. */
int mi355x_vec_lsqr_bidiag(mi355x_handle_t h, size_t n, double coef, const double *coef2_dev, const double *x, double *y, double *out);
int mi355x_vec_lsqr_update(mi355x_handle_t h, size_t n, double ialpha, double step, double cf, double irho2, int skip_w,
                           double *v1, double *x, double *w, double *se);

/* VecMDot_Seq         src/vec/vec/impls/seq/dvec2.c:146     out[j] = sum_i x_i y_j,i , j<nv ; x read once per 16 y's */
int mi355x_vec_mdot(mi355x_handle_t h, size_t n, int nv, const double *x, const double *const *y, double *out);
/* KSPGMRESCycle fusions (gmres.c:118-209, borthog2.c:60-66): x += sum_j sign*coef_dev[j]*y_j in VecMAXPY_Seq's grouping with
 * sum x_new^2 from the same sweep (bits of VecMAXPY + VecNorm); x *= 1/sqrt(*norm2_dev) with VecNormalize's special cases */
int mi355x_vec_maxpy_dev_norm2(mi355x_handle_t h, size_t n, int nv, const double *coef_dev, double sign, const double *const *y,
                               double *x, double *out);
int mi355x_vec_scale_rnorm_dev(mi355x_handle_t h, size_t n, const double *norm2_dev, double *x);
/* KSPFGMRESCycle fusion: mi355x_vec_scale_rnorm_dev (same rules: x is stored unless the norm is 0 or 1 or alpha == 1; alpha == 0 stores
 * zeros) and, from the registers of the same pass, z[i] = x_new[i] * d[i] (d == NULL: z[i] = x_new[i]) for all n entries -- the bits of
 * VecScale followed by VecPointwiseMult (PCApply_Jacobi) or VecCopy (PCApply_None).  One read of n doubles and one launch fewer than
 * the two calls.  hipErrorInvalidValue and nothing touched for a NULL norm2_dev, x or z, and for z == x, z == d or d == x; n == 0 launches
 * nothing.  *norm2_dev may be written by the launch queued before this one on the same stream, not while this one runs. */
int mi355x_vec_scale_rnorm_dev_pmult(mi355x_handle_t h, size_t n, const double *norm2_dev, double *x, const double *d, double *z);
/* VecSum              src/vec/vec/utils/vinv.c (VecSum)    out[0] = sum x_i.  DotF's lanes, order and streaming threshold with
 * y == 1.0: the bits of mi355x_vec_dot(x, ones) for any alignment of x; for a 16-byte aligned x also the bits of the oracle's device-order
 * dot (the oracle restates the aligned tree only; a view off a 16-byte boundary takes the scalar grid-stride loop, another fixed
 * order, within 1e-13 * sum|x_i| of it).  With a null space attached (MatNullSpaceRemove, src/mat/interface/matnull.c)
 * this and the shift below run once per Krylov iteration. */
int mi355x_vec_sum(mi355x_handle_t h, size_t n, const double *x, double *out);
/* VecShift            src/vec/vec/interface/rvector.c      x[i] = x[i] + alpha (no special case for alpha == 0) */
int mi355x_vec_shift(mi355x_handle_t h, size_t n, double alpha, double *x);
/* the same with the shift formed on the device, x[i] = x[i] + (*num_dev / den): num_dev is a sum that never left the device
 * (mi355x_vec_sum into the device scratch); IEEE division, the bits of the host's sum / den */
int mi355x_vec_shift_dev(mi355x_handle_t h, size_t n, const double *num_dev, double den, double *x);
/* VecMax_Seq / VecMin_Seq  src/vec/vec/impls/seq/dvec2.c   out[0] = the extremum, out[1] = its location as a double (exact below
 * 2^53; VecMax_MPI carries it the same way).  What the reference's loop gives -- it starts from x[0] and replaces on a strict > (<):
 * ties return the lowest index and that element's own value (-0.0 against +0.0); a NaN is selected only at position 0 (location 0);
 * n == 0: PETSC_MIN_REAL (PETSC_MAX_REAL for min) and location -1. */
int mi355x_vec_max(mi355x_handle_t h, size_t n, const double *x, double *out);
int mi355x_vec_min(mi355x_handle_t h, size_t n, const double *x, double *out);

/* ---- CSR SpMV (MatMult_SeqAIJ family) --------------------------------- */
/* Analysis: partitions rows into row blocks (<= MI355X_SPMV_BLOCK_NNZ nonzeros staged
 * through LDS per workgroup).  ai_host is the host copy of the row pointer (m+1 ints).
 * If rows_host != NULL the matrix is in compressed-row form (reference:
 * src/mat/utils/compressedrow.c:28): ai_host has nrows+1 entries and rows_host[k]
 * is the output row of compressed row k (device copy kept in the plan). */
int mi355x_spmv_plan_create(mi355x_handle_t h, int nrows, const int *ai_host, const int *rows_host,
                            mi355x_spmv_plan_t *plan);
int mi355x_spmv_plan_destroy(mi355x_spmv_plan_t plan);
/* Optional second analysis step (not for compressed-row plans): if the matrix uses <= 256 distinct offsets
 * (col - row) -- stencil operators -- one byte per nonzero is stored next to the CSR arrays and the SpMV
 * kernels stream val + 1 B instead of val + 4 B col.  Same arithmetic, same bits; no-op otherwise. */
int mi355x_spmv_plan_compress_indices(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai_host, const int *aj_host);
/* row-pattern kernel (stencil matrices: 4 bytes per row instead of 1 byte per nonzero + the row pointer; found by mi355x_spmv_plan_compress_indices):
 * on = 0/1 switches it, on < 0 only asks; *npat = size of the dictionary, 0 when the plan has none */
int mi355x_spmv_plan_use_patterns(mi355x_spmv_plan_t p, int on, int *npat);
/* run-coded row patterns: a row block whose rows form <= 4 runs of equal patterns (a grid line: first, interior, last) is described by
 * one 32-byte descriptor and does not read its rows' words; other blocks keep them.  Same bits.  on = 0/1 switches, on < 0 only asks;
 * *nblocks_run_coded = row blocks described by runs, 0 when the plan has no row patterns */
int mi355x_spmv_plan_use_pattern_runs(mi355x_spmv_plan_t p, int on, int *nblocks_run_coded);
/* The analysis behind it, host arrays only (no device): rowblk = {first row, first nonzero} of nblocks + 1 row blocks, prow[r] =
 * {table start of row r's pattern : 16 (low), first nonzero in its block : 16}, pattab[start] = the pattern's length.
 * runs[8 b + 2 i], runs[8 b + 2 i + 1], i < 4: run i of block b as {prow word of its first row, first row in the block : 16 (low) |
 * length : 16}; unused runs {0, 0xffff}; a block of more than 4 runs has unused runs only. */
int mi355x_spmv_pattern_runs_host(int nblocks, const int *rowblk, const unsigned int *prow, const int *pattab, unsigned int *runs,
                                  int *nblocks_run_coded);
/* value patterns (constant-coefficient operators: whole rows -- offsets AND values, bit for bit -- taken from a table of
 * <= 512 entries; 2 bytes per row, the value array is not read).  _value_patterns derives the table from the host copy of
 * the values that are (about to be) on the device and must be called again after every upload; _drop_ after any change of
 * the device values that did not go through it; _use_: on = 0/1 switches, on < 0 only asks.  *nvpat = distinct rows, 0 =
 * not in use (varying coefficients, compressed-row plan, switched off).  Replaces nothing in the reference: the reference
 * streams MatMult_SeqAIJ's a[] (aij.c:1225); the result carries the same bits. */
int mi355x_spmv_plan_value_patterns(mi355x_handle_t h, mi355x_spmv_plan_t p, const int *ai_host, const int *aj_host,
                                    const double *aa_host, int *nvpat);
int mi355x_spmv_plan_drop_value_patterns(mi355x_spmv_plan_t p);
int mi355x_spmv_plan_use_value_patterns(mi355x_spmv_plan_t p, int on, int *nvpat);
int mi355x_spmv_plan_is_compressed(mi355x_spmv_plan_t plan, int *ntab);
/* 1 when mi355x_spmv_csr_dot would run on this plan with this value array (hipErrorNotSupported otherwise) */
int mi355x_spmv_plan_dot_available(mi355x_spmv_plan_t plan, const double *a, int *yes);
/* Optional analysis step for matrices with repeated row patterns (finite elements with several dof per node): the
 * MI355X form of the reference's inodes.  ns[nnodes] are the node sizes Mat_CheckInode finds (src/mat/impls/aij/seq/
 * inode.c:3981-3998: consecutive rows with identical column lists, <= limit rows per node).  Each group's column list is
 * stored once and the SpMV streams val + (4 / rows-per-group) B instead of val + 4 B per nonzero; `a` stays the CSR
 * array.  No-op (returns 0, plan unchanged) when it would not pay or the plan is compressed-row / index-compressed. */
int mi355x_spmv_plan_group_rows(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai_host, const int *aj_host,
                                int nnodes, const int *ns);
/* Row sums two products at a time, sum += a0 x0 + a1 x1 (MatMult_SeqAIJ_Inode / MatMultAdd_SeqAIJ_Inode, inode.c:430-440,
 * 619-631), instead of one at a time (MatMult_SeqAIJ, aij.h:383-386): set when the reference would run its inode
 * routines on this matrix, so that the result carries ITS rounding.  Applies to the one-lane-per-row paths. */
int mi355x_spmv_plan_set_pairsum(mi355x_spmv_plan_t plan, int on);
int mi355x_spmv_plan_group_info(mi355x_spmv_plan_t plan, int *ngroups, long *nshared_indices, int *pairsum);
int mi355x_spmv_plan_info(mi355x_spmv_plan_t plan, int *nblocks, int *nlong, size_t *workspace_bytes);
/* the device copy of rows_host a compressed-row plan keeps (NULL otherwise; the plan's own, valid while it lives) and the plan's row
 * count: what mi355x_mat_row_reduce takes as `rows` / `mbs` for a matrix whose device row pointer is the compressed one */
int mi355x_spmv_plan_rows(mi355x_spmv_plan_t plan, const int **rows_dev, int *nrows);
/* MatMult_SeqAIJ      src/mat/impls/aij/seq/aij.c:1225 (loop 1269-1277, macro aij.h:383-386)
 *   y[r] = sum_k a[k] x[j[k]], products summed in k order starting from 0.0
 * aa and aj must be allocated with 16 bytes of slack past their last element (mi355x_malloc of nz elements + 16 B):
 * the kernels read aligned pairs, and the pair holding the last element may extend one element past it. */
int mi355x_spmv_csr(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai, const int *aj,
                    const double *aa, const double *x, double *y);
/* y = A x and sum_r x_r y_r from ONE pass over the matrix (KSPSolve_CG: w = A p, dpi = p'w; cg.c:190-191): the SpMV
 * leaves one value per row block in the plan, mi355x_spmv_dot_finish adds them in block order into out[0] (device-
 * accessible).  Square matrices whose plan runs one of the row-block kernels with per-block sums (value patterns, row patterns,
 * 8-bit column offsets: mi355x_spmv_plan_dot_available): mi355x_spmv_csr_dot returns hipErrorNotSupported (801) otherwise and does
 * nothing.  y carries the bits of mi355x_spmv_csr; the dot uses a fixed tree. */
int mi355x_spmv_csr_dot(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai, const int *aj, const double *aa,
                        const double *x, double *y);
int mi355x_spmv_dot_finish(mi355x_handle_t h, mi355x_spmv_plan_t plan, double *out);
/* MatMultAdd_SeqAIJ   src/mat/impls/aij/seq/aij.c:1291   z[r] = y[r] + sum_k ... (sum starts from y[r]);
 * z may alias y.  With a compressed-row plan only the listed rows are touched (z must alias y
 * or already hold y, as aij.c:1314-1316 arranges). */
/* y = d .* (A x): MatMult + PCApply_Jacobi's VecPointwiseMult (jacobi.c:266) in one kernel, bits of the two calls */
int mi355x_spmv_csr_scaled(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai, const int *aj, const double *aa,
                           const double *x, const double *d, double *y);
int mi355x_spmv_csr_add(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai, const int *aj,
                        const double *aa, const double *x, const double *y, double *z);
/* z = d .* (y + A x): one step of a Jacobi-sweep triangular solve with inverted pivots, x^j = dinv .* (y - Us x^(j-1)) with A = -Us
 * (host/ilu.c, -pc_factor_hipmi355x_trisolve sweeps:<k>; mi355x_spmv_csr_add is the step of the unit triangle).  Always the plain
 * row-block kernel.  Short rows: one lane per row, s = y_r, s += a_j x_j in column order, d_r * s, no contraction -- with enough
 * sweeps the bits of MatSolve_SeqAIJ_NaturalOrdering; long rows: the family's lane tree.  z may alias y, x must not alias z;
 * z is stored non-temporally from 256 MiB. */
int mi355x_spmv_csr_add_scaled(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai, const int *aj, const double *aa,
                               const double *x, const double *y, const double *d, double *z);
/* r = b - A x (MatResidual): the row sum mi355x_spmv_csr forms -- from 0.0, in the order of the form the plan runs, pairsum and the
 * long-row lane tree included -- then one subtraction from b_r: the bits of mi355x_spmv_csr(.., w) followed by
 * mi355x_vec_aypx(w, -1, b), empty rows (b_r - 0.0), signed zeros and specials included, without writing and re-reading w.  All five
 * forms mi355x_spmv_csr dispatches (plain, 8-bit offsets, row patterns, value patterns, grouped rows); rectangular plans are fine.
 * r may alias b; x must not alias r (hipErrorInvalidValue, as for a NULL argument).  A compressed-row plan: hipErrorNotSupported
 * (801), nothing written -- those kernels touch the listed rows only. */
int mi355x_spmv_csr_residual(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai, const int *aj, const double *aa,
                             const double *x, const double *b, double *r);
/* MatMultTranspose[Add]_SeqAIJ  src/mat/impls/aij/seq/aij.c:1078-1135 is served by the same two
 * kernels applied to an explicit transpose whose rows list contributions in increasing
 * original-row order (the order the reference's scatter loop adds them in). */

/* MatSetValuesBatch with an unchanged pattern (src/mat/interface/matrix.c:1698; GPU analogue aijAssemble.cu:157):
 * aa[segslot[s]] += v[order[k]] for k in [segptr[s], segptr[s+1]) in that order, s < nseg.  The map is built on the host
 * once per connectivity; contributions are added in the order of the reference's loop of MatSetValues(ADD_VALUES). */
int mi355x_csr_assemble(mi355x_handle_t h, int nseg, const int *segptr, const int *segslot, const int *order, const double *v, double *aa);
/* MatDiagonalScale_SeqAIJ  src/mat/impls/aij/seq/aij.c:2055   a[k] = (a[k] * l[row]) * r[col]; l or r may be NULL */
int mi355x_csr_diagonal_scale(mi355x_handle_t h, int m, const int *ai, const int *aj, double *aa, const double *l, const double *r);
/* MatGetDiagonal_SeqAIJ  src/mat/impls/aij/seq/aij.c:1040   d[r] = A[r,r] or 0 */
int mi355x_csr_get_diagonal(mi355x_handle_t h, int m, const int *ai, const int *aj, const double *aa, double *d);
/* MatShift  src/mat/utils/axpy.c:170   with an unchanged pattern: aa[k] = aa[k] + alpha at the diagonal entry of every row (the row
 * search of mi355x_csr_get_diagonal).  A row without a diagonal entry is not touched; nmissing_dev (device, may be NULL) receives
 * the number of such rows. */
int mi355x_csr_shift(mi355x_handle_t h, int m, const int *ai, const int *aj, double alpha, double *aa, int *nmissing_dev);
/* MatZeroRows_SeqAIJ with MAT_KEEP_NONZERO_PATTERN  aij.c   rows[nrows] (device; duplicates allowed, every row in [0, m)): every stored
 * entry of a listed row is stored as +0.0, its diagonal entry as diag when diag != 0 (-0.0 counts as zero); each entry is written once.
 * x and b (device, both or neither): b[row] = diag * x[row].  nrows <= 0: nothing is launched. */
int mi355x_csr_zero_rows(mi355x_handle_t h, int nrows, const int *rows, const int *ai, const int *aj, double *aa, double diag,
                         const double *x, double *b);
/* The column half of MatZeroRowsColumns_SeqAIJ  aij.c   on a square matrix through its row-block plan (not a compressed-row plan:
 * hipErrorNotSupported).  mask (device): one bit per row = column, bit (c & 31) of word c >> 5, (m + 31) / 32 words, set for the
 * listed ones.  For every row i whose bit is clear, in stored column order, every entry whose column's bit is set: b[i] = b[i] - a_ij *
 * x[col] (two roundings; x and b both or neither), then a_ij = +0.0.  Rows whose bit is set are not touched (mi355x_csr_zero_rows owns
 * them); a row block without such an entry reads its column indices and nothing else.  aj with 16 bytes of slack as for mi355x_spmv_csr. */
int mi355x_csr_zero_columns(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai, const int *aj, double *aa, const unsigned int *mask,
                            const double *x, double *b);
/* MatAXPY_SeqAIJ with SUBSET_NONZERO_PATTERN  aij.c:2621   ya[xtoy[k]] = ya[xtoy[k]] + alpha * xa[k], k < nzx, two roundings;
 * xtoy injective (no atomics); alpha == 0 does the arithmetic too (the same-pattern form, mi355x_vec_axpy on the value arrays,
 * returns at once as daxpy does); same-pattern MatCopy is mi355x_memcpy_d2d.  xa may be ya with the identity map. */
int mi355x_csr_axpy_map(mi355x_handle_t h, int nzx, const int *xtoy, double alpha, const double *xa, double *ya);
/* the map of that update (host only, no device call): for every stored entry k of X, m rows, xtoy[k] = position of the same (row,
 * column) in Y; the columns of a row ascending in both.  xcols / ycols (may be NULL): local -> global column translations, increasing
 * (the off-diagonal blocks of MPIAIJ, compacted through each matrix's own garray).  X stores an entry Y lacks: non-zero, the first
 * such row in *bad_row (-1 otherwise), xtoy undefined.  Rows are split over host threads from 200 000 entries. */
int mi355x_csr_subset_map(int m, const int *xi, const int *xj, const int *xcols, const int *yi, const int *yj, const int *ycols, int *xtoy, int *bad_row);

/* ---- row reductions over the stored values (csrc/mat_reduce.hip) ------- */
/* MatNorm_SeqAIJ / MatGetRowMaxAbs_SeqAIJ / MatGetRowMax_SeqAIJ / MatGetRowMin_SeqAIJ (aij.c), MatNorm_SeqBAIJ (baij.c): one result per
 * point row of a CSR (bs = 1) or BCSR (bs = 2 .. 7, blocks column-major) matrix of mbs block rows and ncols scalar columns.  A point
 * row's entries are taken in storage order -- block after block, a block's columns left to right -- by one lane, so every result
 * carries the bits of the sequential loop:
 *   MI355X_ROW_SUM / _ABSSUM / _SQSUM   s = acc ? acc[row] : 0.0; then s = s + a, s + |a|, s + a * a (product and sum rounded separately)
 *                                       entry by entry.  acc (may be NULL, may be out) continues a sum: the off-diagonal block of an
 *                                       MPIAIJ row after its diagonal block.
 *   MI355X_ROW_MAXABS                   starts at (0.0, column 0); an entry replaces the current value on cur < |a| only: the first of
 *                                       equals stays, a NaN never replaces and is never replaced.
 *   MI355X_ROW_MAX / _MIN               a row that stores fewer than ncols entries starts at the implicit (0.0, the smallest column
 *                                       the row does not store -- columns ascending within the row), a full row at its first entry, a
 *                                       row without entries gives (0.0, 0); replacement on cur < a (a < cur) only.
 * out[row] gets the value, idx[row] (extrema only; may be NULL; needs aj) the scalar column.  rows (bs = 1 only, may be NULL): the
 * compressed-row form, row r of ai is row rows[r] of acc / out / idx and no other row is written.  Value offsets are 32-bit:
 * ai[mbs] bs^2 < 2^31.  All arrays on the device.  Nothing outside out[0, mbs bs) / idx[0, mbs bs) is written; empty rows are legal.
 * The maximum or the sum over the results is mi355x_vec_max / mi355x_vec_norm on out. */
#define MI355X_ROW_SUM    0
#define MI355X_ROW_ABSSUM 1
#define MI355X_ROW_SQSUM  2
#define MI355X_ROW_MAXABS 3
#define MI355X_ROW_MAX    4
#define MI355X_ROW_MIN    5
int mi355x_mat_row_reduce(mi355x_handle_t h, int op, int mbs, int bs, int ncols, const int *ai, const int *aj, const double *aa,
                          const int *rows, const double *acc, double *out, int *idx);

/* ---- column-tiled CSR SpMV: x staged in LDS (csrc/spmv_tiled.hip) ------ */
/* For matrices whose x gathers miss the caches (rows that pick columns from a wide window without neighbouring rows sharing them):
 * MatMult_SeqAIJ / MatMultAdd_SeqAIJ (aij.c:1225, 1291) re-cut into row panels (<= 6143 rows, equal shares of the nonzeros) x column
 * tiles of 2048 entries of x; a (panel, tile) pair with >= stage_min entries gathers from a copy of that tile in LDS and adds into row
 * sums that live in LDS too (12-byte entries in dense blocks of 128, two per lane, ds_add_f64); the thin pairs' entries (the remainder)
 * follow in the same streams, grouped by windows of 2^18 columns, their x gathered from global memory -- one kernel, y written once.
 * Products of a row's staged entries are added in column order, then the remainder's in column order: agrees with the reference to
 * rounding (<= 1e-12 * sum |a_ij x_j|; bit for bit when nothing or everything is left to the remainder), reproducible.
 *   _probe    fraction of sampled gathers that touch a 128-byte line of x nothing else in their 32-row group touches (host only)
 *   _build    the layout from the host CSR pattern (host only: no device call); stage_min <= 0: 1024
 *   _upload   tables to the device; values gathered from the CSR value array that is on the device (aa_dev)
 *   _refresh_values   after the device values changed under the same pattern
 *   mi355x_spmv_tiled  yout = (yin ? yin : 0) + A x; x 16-byte aligned, else hipErrorNotSupported (801) and nothing is launched */
typedef struct mi355x_spmv_tiled_s *mi355x_spmv_tiled_t;
int mi355x_spmv_tiled_probe(int m, const int *ai_host, const int *aj_host, double *lines_per_nonzero);
int mi355x_spmv_tiled_build(int m, int n, const int *ai_host, const int *aj_host, int stage_min, mi355x_spmv_tiled_t *plan);
/* nblocks: 128-entry blocks stored over all wavefronts (nnz_staged / (128 nblocks): the share that is not padding) */
int mi355x_spmv_tiled_info(mi355x_spmv_tiled_t plan, long *nnz_staged, long *nnz_remainder, int *npanels, int *npairs, long *nblocks);
int mi355x_spmv_tiled_geometry(int *panel_rows, int *tile_cols, int *waves, int *block_entries);
int mi355x_spmv_tiled_upload(mi355x_handle_t h, mi355x_spmv_tiled_t plan, const double *aa_dev);
int mi355x_spmv_tiled_refresh_values(mi355x_handle_t h, mi355x_spmv_tiled_t plan, const double *aa_dev);
int mi355x_spmv_tiled(mi355x_handle_t h, mi355x_spmv_tiled_t plan, const double *x, const double *yin, double *yout);
/* development: which = 1 the staged part only, 2 the remainder only (their separate cost), 0 both */
int mi355x_spmv_tiled_parts(mi355x_handle_t h, mi355x_spmv_tiled_t plan, const double *x, const double *yin, double *yout, int which);
/* tests: one host array of the layout (0 pt_ptr, 1 pt_tile, 2 pw_e0, 3 word, 4 perm, 7 pw_f0, 8 fw_ptr, 9 fw_win, 10 wrow, 11 prow)
 * until _drop_host releases the host copy */
int mi355x_spmv_tiled_debug_get(mi355x_spmv_tiled_t plan, int which, void *out, size_t cap_bytes, size_t *bytes);
int mi355x_spmv_tiled_drop_host(mi355x_spmv_tiled_t plan);
int mi355x_spmv_tiled_destroy(mi355x_spmv_tiled_t plan);

/* ---- BCSR SpMV (MatMult_SeqBAIJ_3/_4/_N) ------------------------------- */
/* src/mat/impls/baij/seq/baij2.c:331 (bs=3), :387 (bs=4), :981 (N); blocks column-major */
int mi355x_spmv_bsr(mi355x_handle_t h, int mbs, int bs, const int *ai, const int *aj,
                    const double *aa, const double *x, double *y);          /* one wavefront per block row, no analysis */
/* row-block streaming variant: `plan` = mi355x_spmv_plan_create over the block-row pointer multiplied by bs*bs
 * (it then partitions by VALUES); aligned 16-byte loads need aa 16-byte aligned */
int mi355x_spmv_bsr_planned(mi355x_handle_t h, mi355x_spmv_plan_t plan, int bs, const int *ai, const int *aj,
                            const double *aa, const double *x, double *y);
/* MatMultAdd_SeqBAIJ_3/_4/_N  src/mat/impls/baij/seq/baij2.c:1168-1480   z = y + A x with the same kernel; z may alias y */
int mi355x_spmv_bsr_planned_add(mi355x_handle_t h, mi355x_spmv_plan_t plan, int bs, const int *ai, const int *aj,
                                const double *aa, const double *x, const double *y, double *z);
/* the same product with the row-block kernel's form chosen by the caller (development / A-B runs): x_in_lds != 0 stages the x
 * entries of the row block's block columns in LDS once per block instead of gathering them once per value */
int mi355x_spmv_bsr_planned_form(mi355x_handle_t h, mi355x_spmv_plan_t plan, int bs, int x_in_lds, const int *ai, const int *aj,
                                 const double *aa, const double *x, double *y);

/* bs = 4 on the matrix cores (v_mfma_f64_4x4x4_4b_f64 as a fused multiply + 4-lane reduction; BASELINE configs[4]); one
 * wavefront per block row, no analysis.  variant 0: 16-byte loads (8 blocks per step), 1: 8-byte loads (4 per step).
 * FMA arithmetic and a tree over the four block columns: agrees with MatMult_SeqBAIJ_4 (baij2.c:387) to rounding. */
int mi355x_spmv_bsr4_mfma(mi355x_handle_t h, int mbs, int variant, const int *ai, const int *aj, const double *aa,
                          const double *x, double *y);

/* PCApply_PBJacobi_N  src/ksp/pc/impls/pbjacobi/pbjacobi.c:20-200   y_i = D_i^-1 x_i, idiag = mbs inverted bs x bs blocks
 * (column-major, as MatInvertBlockDiagonal_SeqBAIJ baij.c:13 leaves them); the reference's left-to-right row sums */
int mi355x_pbjacobi_apply(mi355x_handle_t h, int mbs, int bs, const double *idiag, const double *x, double *y);

/* ---- ILU(0) triangular solves ---------------------------- */
/* MatSolve_SeqAIJ_NaturalOrdering  src/mat/impls/aij/seq/aijfact.c:3126-3172 on the factor layout of :1628-1700,
 * one launch per dependency level; `rows` lists the rows of the level (device array).  Lower: x[i] = b[i] - L(i,:)x
 * (b may alias x); upper: x[i] = (x[i] - U(i,:)x) * inverted diagonal. */
int mi355x_ilu0_lower_level(mi355x_handle_t h, int nrows, const int *rows, const int *bi, const int *bj,
                            const double *ba, const double *b, double *x);
int mi355x_ilu0_upper_level(mi355x_handle_t h, int nrows, const int *rows, const int *bj, const double *ba,
                            const int *bdiag, double *x);

/* ---- transposed triangular solves of the same factors (csrc/trisolve_transpose.hip) ----
 * MatSolveTranspose_SeqAIJ  src/mat/impls/aij/seq/aijfact.c with the natural ordering: the forward solve with U^T (scaled by the inverted
 * diagonal), then the backward solve with L^T (unit diagonal).  The device runs the GATHER form over the transposed triangles, stored as
 * two CSR triangles whose rows are in the order the reference's scatter loop reaches an entry: U^T's row c lists the rows i < c of U that
 * hold column c ASCENDING, L^T's row c the rows i > c of L DESCENDING.  One launch per dependency level, `rows` the level's rows (device
 * array), one lane per row, the row walked in storage order, every product rounded before its subtraction: x carries the loop's bits.
 *   _first_level   x[c] = (b[c] - ta[q] x[tj[q]] - ...) * dinv[c] over q = ti[c] .. ti[c + 1] - 1.  b may alias x.
 *   _second_level  x[c] =  x[c] - sa[q] x[sj[q]] - ...            over q = si[c] .. si[c + 1] - 1, in place.
 *   nrows <= 0 launches nothing.  No hand-off between workgroups: the kernel boundary between levels is the only synchronisation.
 *   _build_host    HOST arrays, no device call, one thread: from the factor's bi / bj / bdiag the two patterns (ti, si: n + 1 ints; tj,
 *             tperm: one int per strict-upper entry, bdiag[0] + 1 - bi[n] - n of them; sj, sperm: bi[n] ints), tperm / sperm the position in
 *             ba of every value (the inverted diagonal of row c is ba[bdiag[c]]; mi355x_pack gathers values through such a list on the
 *             device), and the dependency level of every row of each triangle: 0 for a row without entries, else one more than the
 *             deepest row it reads; *nlev_* = levels, every one of them non-empty (0 for n == 0).  hipErrorInvalidValue for a layout
 *             that is not the one above (a column on the wrong side of the diagonal or outside the matrix, pointers that do not
 *             increase) or a missing array; nothing is thrown across this interface. */
int mi355x_ilut_first_level(mi355x_handle_t h, int nrows, const int *rows, const int *ti, const int *tj, const double *ta,
                            const double *dinv, const double *b, double *x);
int mi355x_ilut_second_level(mi355x_handle_t h, int nrows, const int *rows, const int *si, const int *sj, const double *sa, double *x);
int mi355x_ilut_build_host(int n, const int *bi, const int *bj, const int *bdiag, int *ti, int *tj, int *tperm, int *si, int *sj,
                           int *sperm, int *levT_first, int *nlev_first, int *levT_second, int *nlev_second);

/* ---- ILU(0) numeric factorisation, level by level (csrc/ilu_factor.hip) ------------------------------------------------------
 * MatLUFactorNumeric_SeqAIJ  src/mat/impls/aij/seq/aijfact.c:505-570 with the restarts of MatPivotCheck_nz (matimpl.h:512-528), on
 * the layout of MatILUFactorSymbolic_SeqAIJ_ilu0 (:1628-1700): one launch per dependency level of L, a power-of-two number of lanes
 * per row (chosen from the widest row), every row's arithmetic the sequential loop's -- ba carries the reference's bits.
 *   _create   once per pattern, from HOST arrays: the factor's bi / bj / bdiag, the rows sorted by dependency level of L (levptr[nlev + 1],
 *             rows[n]), the independent blocks (blk[nblk + 1] row ranges; nblk <= 1: one block).  The layout is checked
 *             (hipErrorInvalidValue); a creator that fails frees what it allocated.
 *   _reset    a new numeric factorisation starts: every block is pending again
 *   _run      one pass over the blocks still pending.  ai / aj / aa: A's CSR on the device (the pattern the factor's was taken from),
 *             ba: the factor's nz + 1 values on the device, shift_per_block[nblk] (host) the diagonal shifts.  Returns after one host
 *             wait with failed_row[b] (host; -1: the block passed and is no longer pending) and failed_abs[b] = |pivot| of that row.
 *   _arrays   the context's device copies (bi, bj, bdiag, rows in level order), borrowed: they live as long as the context
 *   _to_sweeps  the sweep form of the factor (mi355x_spmv_csr_add / _add_scaled above): aL = -ba over the L part, aU / dinv through
 *             the row pointers iU (device) of the strict upper triangle as CSR
 *   _info     lanes per row, levels */
typedef struct mi355x_ilu0_factor_s *mi355x_ilu0_factor_t;
int mi355x_ilu0_factor_create(mi355x_handle_t h, int n, const int *bi, const int *bj, const int *bdiag, int nlev, const int *levptr,
                              const int *rows, int nblk, const int *blk, mi355x_ilu0_factor_t *ctx);
int mi355x_ilu0_factor_destroy(mi355x_ilu0_factor_t ctx);
int mi355x_ilu0_factor_reset(mi355x_ilu0_factor_t ctx);
int mi355x_ilu0_factor_run(mi355x_handle_t h, mi355x_ilu0_factor_t ctx, const int *ai, const int *aj, const double *aa, double zeropivot,
                           const double *shift_per_block, double *ba, int *failed_row, double *failed_abs);
int mi355x_ilu0_factor_arrays(mi355x_ilu0_factor_t ctx, const int **bi, const int **bj, const int **bdiag, const int **rows);
int mi355x_ilu0_factor_to_sweeps(mi355x_handle_t h, mi355x_ilu0_factor_t ctx, const int *iU, const double *ba, double *aL, double *aU, double *dinv);
int mi355x_ilu0_factor_info(mi355x_ilu0_factor_t ctx, int *lanes, int *nlev);

/* ---- ILU(k): level-of-fill pattern on the host, numeric factorisation on a pattern with fill on the device (csrc/ilu_factor.hip) ----
 * MatILUFactorSymbolic_SeqAIJ with natural ordering, in the layout of MatILUFactorSymbolic_SeqAIJ_ilu0 that everything above reads (L rows
 * forward from bi, U rows stored from the last row backwards, the diagonal at bdiag[i], bdiag[n] = bi[n] - 1).
 *   _iluk_symbolic_host  host arrays, no device call, one thread (row i reads the levels of the U rows before it).  A stored a_ij has
 *             level 0; row i is built from the sorted list of its columns: for every list column k < i in ascending order, fill that
 *             entered earlier included, incr = lev(i,k) + 1 and every strict-upper entry (k,j) of row k with lev(k,j) + incr <= levels
 *             enters the list with that level (an entry already there keeps the smaller one).  levels == 0 is A's own pattern.
 *             Called twice: with bj == NULL it fills bi[n + 1] and bdiag[n + 1]; with bj (and those two arrays as the first call left
 *             them) it fills the columns and, with bjlev (may be NULL), every stored entry's level.  bj and bjlev hold bdiag[0] + 2
 *             ints; the last one is not written.  hipErrorInvalidValue with *bad_row (may be NULL; -1 when no row is at fault) for an
 *             empty row, a row without its diagonal entry, unsorted columns or columns outside the matrix, and for levels < 0.
 *   _create_fill  mi355x_ilu0_factor_create for a factor pattern that contains A's: ai_host / aj_host are A's pattern (host).  The
 *             same layout checks, and every row of A must be a sorted subset of its factor row (hipErrorInvalidValue).  The lanes per
 *             row come from the widest FACTOR row.  The context serves _reset / _run / _arrays / _to_sweeps / _info / _destroy as
 *             above; _run then starts every work row from A's entry at the factor's column or +0.0 where A stores none, skips a
 *             multiplier that is == 0.0 (a fill entry nothing has touched included), and leaves the sequential loop's bits in ba
 *             (bdiag[0] + 2 doubles, the last one never written). */
int mi355x_iluk_symbolic_host(int n, const int *ai, const int *aj, int levels, int *bi, int *bdiag, int *bj, int *bjlev, int *bad_row);
int mi355x_ilu0_factor_create_fill(mi355x_handle_t h, int n, const int *ai_host, const int *aj_host, const int *bi, const int *bj,
                                   const int *bdiag, int nlev, const int *levptr, const int *rows, int nblk, const int *blk,
                                   mi355x_ilu0_factor_t *ctx);

/* ---- Block ILU(k) of a BAIJ matrix: level-scheduled block triangular solves, host numeric factorisation (csrc/bilu.hip) ----
 * MatSolve_SeqBAIJ_<bs>_NaturalOrdering  src/mat/impls/baij/seq/baijfact2.c on the point factor's layout over BLOCK rows and columns (bi,
 * bj, bdiag as above; mi355x_iluk_symbolic_host on the block pattern builds it) with ba holding one column-major bs x bs block per
 * stored entry and the INVERTED diagonal block at bdiag[i], 2 <= bs <= 7.  One launch per dependency level, `rows` the block rows of
 * the level (device array); one lane per scalar row, the bs lanes of a block row in one wavefront.  Or one launch for a run of
 * consecutive levels (_chain), the same arithmetic in the same order: the two ways give the same bits.
 *   _lower_level  component r of block row i: s = b[bs i + r]; for every stored L block (i,k) in storage order, with v the block and
 *             x_k the solution of block row k, s = s - (v[r] x_k[0] + v[r + bs] x_k[1] + ... + v[r + (bs-1) bs] x_k[bs-1]) -- the
 *             products summed left to right, then one subtraction; x[bs i + r] = s.  b may alias x.
 *   _upper_level  the same accumulation over the strict-upper blocks bdiag[i+1]+1 .. bdiag[i]-1 starting from x[bs i + r], then
 *             x[bs i + r] = d[r] s_0 + d[r + bs] s_1 + ... left to right, d the inverted diagonal block, s_c the sums of the row's
 *             bs components.
 *   bs outside 2..7: hipErrorInvalidValue, nothing launched.  nrows <= 0 launches nothing.  Padding lanes and rows past nrows neither
 *   load nor store.  No hand-off between workgroups: the kernel boundary between levels is the only synchronisation.
 *   _lower_chain / _upper_chain  nlev consecutive levels in ONE launch of ONE workgroup of 1024 threads: level l is the block rows
 *             rows[levptr[l]] .. rows[levptr[l+1] - 1] (levptr: nlev + 1 non-decreasing offsets into rows, a DEVICE array; a sub-range
 *             of a factor's levels is levptr + l0 with nlev = l1 - l0 and the same rows).  The workgroup takes a level 1024 / W block
 *             rows at a time (W = 2, 4, 8 lanes for bs = 2, 3..4, 5..7), each pass the body of the level kernel, then ONE
 *             __syncthreads() per level; an empty level costs that barrier.  x is written with plain stores and read behind the
 *             barrier by waves of the same workgroup: no hand-off between workgroups, no polling, no atomics, nothing that can
 *             hang.  Worth it for levels too narrow to fill more than one CU; a wide level wants _level's grid.  b may alias x in
 *             _lower_chain.  bs outside 2..7: hipErrorInvalidValue, nothing launched; nlev <= 0 launches nothing.
 *   _chain_plan_host  which levels to chain, on HOST arrays, no device call: a level is narrow when it has at most max_rows block
 *             rows (max_rows <= 0: no level is).  [0, nlev) is cut into *nseg segments seg_ptr[s] .. seg_ptr[s+1] - 1 in order: every
 *             maximal run of narrow levels is one segment with seg_fused[s] = 1 (a run of one level included), every wide level
 *             a segment of its own with seg_fused[s] = 0.  seg_ptr holds nlev + 1 ints, seg_fused nlev.  nlev = 0: *nseg = 0, the
 *             arrays untouched.  hipErrorInvalidValue for nlev < 0, a NULL array with nlev > 0, a NULL nseg, a decreasing levptr.
 *   _numeric_host  MatLUFactorNumeric_SeqBAIJ_<bs>_NaturalOrdering restated on HOST arrays, one thread, no device call: A's block
 *             CSR (ai, aj, aa; mbs block rows) into ba on a factor pattern that contains A's.  Block row i: every work block of the
 *             factor row starts at +0.0 with A's blocks copied in; for every L block (i,k) in ascending k, fill included, that is not
 *             entirely == 0.0: M = W_k D_k^-1, stored as the L block, and W_j = W_j - M U_kj for every strict-upper block (k,j) of
 *             row k whose column the factor row i holds -- every entry of a block product a left-to-right sum of bs products, then
 *             one subtraction; the L and U blocks are stored; D_i^-1 by LINPACK dgefa + dgedi (mi355x_block_inverse.h) in the
 *             diagonal's slot.  A zero pivot there: hipErrorUnknown with the scalar row in *zero_pivot_row (may be NULL; -1
 *             otherwise) and the block rows before it as computed.  hipErrorInvalidValue for bs outside 2..7, a NULL array, a factor
 *             row whose diagonal slot does not name the row, and a block of A the factor's pattern lacks. */
int mi355x_bilu_lower_level(mi355x_handle_t h, int nrows, const int *rows, int bs, const int *bi, const int *bj, const double *ba,
                            const double *b, double *x);
int mi355x_bilu_upper_level(mi355x_handle_t h, int nrows, const int *rows, int bs, const int *bj, const double *ba, const int *bdiag,
                            double *x);
int mi355x_bilu_lower_chain(mi355x_handle_t h, int nlev, const int *levptr, const int *rows, int bs, const int *bi, const int *bj,
                            const double *ba, const double *b, double *x);
int mi355x_bilu_upper_chain(mi355x_handle_t h, int nlev, const int *levptr, const int *rows, int bs, const int *bj, const double *ba,
                            const int *bdiag, double *x);
int mi355x_bilu_chain_plan_host(int nlev, const int *levptr, int max_rows, int *seg_ptr, int *seg_fused, int *nseg);
int mi355x_bilu_numeric_host(int mbs, int bs, const int *ai, const int *aj, const double *aa, const int *bi, const int *bj,
                             const int *bdiag, double *ba, int *zero_pivot_row);

/* ---- SOR / SSOR sweeps on a square CSR matrix as it is (csrc/sor.hip) ----
 * MatSOR_SeqAIJ  src/mat/impls/aij/seq/aij.c:1463 with the point sweeps (never the inode routine), level by level: one lane per row, a
 * row's products subtracted in storage order, each product and each difference rounded -- x carries the sequential loop's bits.
 *   _levels_host  lev[i] = 0, or 1 + max lev[j] over the j < i with a(i,j) OR a(j,i) stored (the pattern of A + A^T); *nlev = levels.
 *             Host arrays, no device.  Every coupled pair j < i has lev[j] < lev[i]: ascending levels are a forward sweep, descending
 *             levels a backward one (why one set serves both: csrc/sor.hip).
 *   _plan_create  once per pattern, from HOST ai / aj: checks the pattern (m >= 0, ai increasing from 0, every row's columns strictly
 *             increasing and inside [0, m), a stored diagonal in every row: hipErrorInvalidValue, *bad_row -- may be NULL -- the first
 *             offending row or -1), then the levels, the rows in level order and every row's diagonal position, on the device.
 *             A maximal run of consecutive levels of at most 256 rows each becomes ONE launch of one workgroup that walks the run's
 *             levels with a barrier between them; MI355X_SOR_NO_FUSE in flags gives every level its own launch.  Same bits either way.
 *   _plan_info    levels, launches per sweep (either direction), levels that sit inside fused runs
 *   _idiag    mdiag[i] = a(i,i); idiag[i] = 1 / a(i,i) when omega == 1 and fshift == 0, else omega / (fshift + a(i,i))
 *   _sweep    one sweep of one kind over the device CSR arrays (the pattern the plan was made from):
 *               ZERO_FORWARD         sum = b[i] - sum_{j<i} a_ij x[j];  t[i] = sum;  x[i] = sum idiag[i]                 (levels ascending)
 *               ZERO_BACKWARD        sum = b[i] - sum_{j>i} a_ij x[j];  x[i] = sum idiag[i]                             (descending)
 *               ZERO_BACKWARD_AFTER  sum = t[i] - sum_{j>i} a_ij x[j];  x[i] = (1 - omega) x[i] + sum idiag[i]          (descending)
 *               FORWARD / BACKWARD   sum = b[i] - sum_j a_ij x[j];  x[i] = (1 - omega) x[i] + (sum + mdiag[i] x[i]) idiag[i]
 *             t may be NULL for the kinds that do not touch it.  b and x must not overlap.
 *   _apply    the whole of MatSOR_SeqAIJ after its checks: flag is a MatSORType bit set (FORWARD 1, BACKWARD 2, LOCAL_FORWARD 4,
 *             LOCAL_BACKWARD 8, ZERO_INITIAL_GUESS 16; any other bit: hipErrorInvalidValue), its > 0 the product its * lits.
 * Nothing here waits for the device. */
typedef struct mi355x_sor_plan_s *mi355x_sor_plan_t;
enum { MI355X_SOR_ZERO_FORWARD = 0, MI355X_SOR_ZERO_BACKWARD = 1, MI355X_SOR_ZERO_BACKWARD_AFTER = 2, MI355X_SOR_FORWARD = 3, MI355X_SOR_BACKWARD = 4 };
#define MI355X_SOR_NO_FUSE 1
int mi355x_sor_levels_host(int m, const int *ai, const int *aj, int *lev, int *nlev);
int mi355x_sor_plan_create(mi355x_handle_t h, int m, const int *ai, const int *aj, int flags, mi355x_sor_plan_t *plan, int *bad_row);
int mi355x_sor_plan_destroy(mi355x_sor_plan_t plan);
int mi355x_sor_plan_info(mi355x_sor_plan_t plan, int *nlev, int *launches_per_sweep, int *fused_levels);
int mi355x_sor_idiag(mi355x_handle_t h, mi355x_sor_plan_t plan, const double *aa, double omega, double fshift, double *idiag, double *mdiag);
int mi355x_sor_sweep(mi355x_handle_t h, mi355x_sor_plan_t plan, int kind, const int *ai, const int *aj, const double *aa, const double *idiag,
                     const double *mdiag, double omega, const double *b, double *t, double *x);
int mi355x_sor_apply(mi355x_handle_t h, mi355x_sor_plan_t plan, const int *ai, const int *aj, const double *aa, const double *idiag,
                     const double *mdiag, double omega, int flag, int its, const double *b, double *t, double *x);

/* ---- C = A B for CSR matrices: symbolic pass on the host, numeric pass on the device (csrc/spgemm.hip) ----
 * MatMatMult_SeqAIJ_SeqAIJ  src/mat/impls/aij/seq/matmatmult.c.  A is m x k, B is k x n, every row's columns ascending.  Row i of C
 * stores the union of the column lists of the rows B[aj[t], :], t over row i of A, ascending, also where a value comes out zero.
 * Every c_ij starts at +0.0; the stored entries t of A's row i are taken in storage order and every stored b = B[aj[t], j] gives
 * c_ij = c_ij + (a_it * b), product and sum rounded separately; nothing is skipped (a stored 0.0 against an Inf is a NaN).  C carries
 * the sequential loop's bits whatever the lane width and launch shape.
 *   _symbolic_host  host arrays, no device call; called twice: with cj == NULL it fills ci[m + 1], with cj it fills the sorted columns
 *             at the offsets of ci.  Rows are split over nthreads host threads (<= 0: one below 200 000 entries of A, else
 *             mi355x_host_threads(16)); the result does not depend on the count.
 *   _geometry     the LDS slots a row of C has before it is processed in column windows, and the workgroup size
 *   _plan_create  once per pattern triple, from HOST arrays: checks them (row pointers ascending from 0, columns strictly ascending
 *             and inside their matrix: hipErrorInvalidValue), picks the lanes per row -- the smallest of 8, 16, 32, 64 that is >= the
 *             mean length of the B rows the product visits -- and uploads the list of C's non-empty rows, the windowed ones last
 *   _plan_info    lanes per row, rows of C longer than the LDS budget, bytes of device memory the plan holds
 *   _numeric      DEVICE arrays of the patterns the plan was made from: writes every one of the ci[m] slots of ca and nothing else;
 *             does not wait for the device */
typedef struct mi355x_spgemm_plan_s *mi355x_spgemm_plan_t;
int mi355x_spgemm_symbolic_host(int m, int n, const int *ai, const int *aj, const int *bi, const int *bj, int *ci, int *cj, int nthreads);
int mi355x_spgemm_geometry(int *lds_entries_per_row_group, int *block);
int mi355x_spgemm_plan_create(mi355x_handle_t h, int m, int k, int n, const int *ai, const int *aj, const int *bi, const int *bj, const int *ci,
                              const int *cj, mi355x_spgemm_plan_t *plan);
int mi355x_spgemm_plan_destroy(mi355x_spgemm_plan_t plan);
int mi355x_spgemm_plan_info(mi355x_spgemm_plan_t plan, int *lanes, int *nwindowed_rows, size_t *workspace_bytes);
int mi355x_spgemm_numeric(mi355x_handle_t h, mi355x_spgemm_plan_t plan, const int *ai, const int *aj, const double *aa, const int *bi,
                          const int *bj, const double *ba, const int *ci, const int *cj, double *ca);

/* The same two solves WITHOUT a kernel boundary per level: one launch per triangular solve, rows sorted by level and
 * stored as sliced ELL (one wavefront per 64 rows), dependencies handed over through the solution values themselves
 * (a sentinel bit pattern means "not computed yet"; write-through stores, polling loads).  Same one-lane-per-row,
 * column-order arithmetic: same bits.  plan_create: lev[i] = dependency level of row i (every level non-empty), row i's
 * off-diagonal entries are cj/cv[rp[i] .. rp[i]+rl[i]), dinv != NULL (inverted diagonal per row) marks the upper solve.
 * apply: y = U^-1 L^-1 b; returns non-zero without launching if an earlier application timed out on a dependency.  A NaN is a
 * solution value like any other, except the one bit pattern of the sentinel (0xFFF8DEADBEEFCAFE): a solution value with exactly
 * those bits cannot be told from "not computed yet" -- its consumers wait until they give up and the application aborts. */
typedef struct mi355x_trisolve_plan_s *mi355x_trisolve_plan_t;
int mi355x_trisolve_plan_create(mi355x_handle_t h, int n, int nlev, const int *lev, const int *rp, const int *rl, const int *cj,
                                const double *cv, const double *dinv, mi355x_trisolve_plan_t *plan);
/* by_level != 0: rows summed in the order of their dependencies' levels instead of column order (factors of inode matrices;
 * tolerance instead of bit-exactness against MatSolve_SeqAIJ_NaturalOrdering), large levels on slice boundaries */
int mi355x_trisolve_plan_create_ordered(mi355x_handle_t h, int n, int nlev, const int *lev, const int *rp, const int *rl, const int *cj,
                                        const double *cv, const double *dinv, int by_level, mi355x_trisolve_plan_t *plan);
/* upper solve of an incomplete Cholesky factor U^T D U: right-hand side entry i is multiplied by rscale[i] (= 1/D(i)) before row
 * i's sum starts -- the x[i] = xi * (1/D(i)) between the two sweeps of MatSolve_SeqSBAIJ_1_NaturalOrdering (sbaijfact2.c:1977-2015);
 * entries in the caller's order */
int mi355x_trisolve_plan_create_scaled(mi355x_handle_t h, int n, int nlev, const int *lev, const int *rp, const int *rl, const int *cj,
                                       const double *cv, const double *dinv, const double *rscale, mi355x_trisolve_plan_t *plan);
/* node-blocked plans for the factor of a matrix with inodes (MatSolve_SeqAIJ_Inode, src/mat/impls/aij/seq/inode.c:2327-2760): the
 * n rows form nnodes nodes of 1..5 consecutive rows (nstart[nnodes + 1]) whose factor rows share one column list and are coupled by a
 * dense triangle; nodelev[u] = dependency level of node u among the nodes.  Row-level arrays as above, in the reference's stored order.
 * One lane per node; the reference routine's summation order (shared columns two at a time, then the couplings inside the node):
 * bit for bit MatSolve_SeqAIJ_Inode with by_level == 0.  Returns hipErrorInvalidValue for a factor without that shape.  Lower and
 * upper plan of an application must both be node plans of the same partition and the same block_columns.
 * block_columns != 0: additionally every node has the same number of rows (<= 4) and every shared column list is a run of WHOLE
 * dependency nodes (a FEM matrix with a fixed number of dofs per node): one list entry and one contiguous gather per dependency node
 * -- fewer, larger batches; same column sequence, same bits.  hipErrorInvalidValue when the factor is not of that kind. */
int mi355x_trisolve_plan_create_nodes(mi355x_handle_t h, int n, int nnodes, const int *nstart, int nlev, const int *nodelev, const int *rp, const int *rl,
                                      const int *cj, const double *cv, const double *dinv, int by_level, int block_columns, mi355x_trisolve_plan_t *plan);
/* the lower and the upper row-granular plan of one factor, built side by side (two host threads): the arguments of
 * mi355x_trisolve_plan_create_ordered for the lower plan, of ..._create_ordered / ..._create_scaled (rscale_up != NULL) for the upper
 * one; on failure neither plan is returned */
int mi355x_trisolve_plan_create_pair(mi355x_handle_t h, int n, int by_level,
                                     int nlev_lo, const int *lev_lo, const int *rp_lo, const int *rl_lo, const int *cj_lo, const double *cv_lo,
                                     int nlev_up, const int *lev_up, const int *rp_up, const int *rl_up, const int *cj_up, const double *cv_up,
                                     const double *dinv_up, const double *rscale_up, mi355x_trisolve_plan_t *lower, mi355x_trisolve_plan_t *upper);
/* the lower and the upper node plan of one factor, built side by side (two host threads: the analyses are independent): arguments as
 * above, once per factor; on failure neither plan is returned */
int mi355x_trisolve_plan_create_nodes_pair(mi355x_handle_t h, int n, int nnodes, const int *nstart, int by_level, int block_columns,
                                           int nlev_lo, const int *nodelev_lo, const int *rp_lo, const int *rl_lo,
                                           int nlev_up, const int *nodelev_up, const int *rp_up, const int *rl_up,
                                           const int *cj, const double *cv, const double *dinv, mi355x_trisolve_plan_t *lower, mi355x_trisolve_plan_t *upper);
int mi355x_trisolve_plan_destroy(mi355x_trisolve_plan_t plan);
int mi355x_trisolve_apply(mi355x_handle_t h, mi355x_trisolve_plan_t lower, mi355x_trisolve_plan_t upper, const double *b, double *y);
int mi355x_trisolve_aborted(mi355x_trisolve_plan_t plan, int *aborted);
/* tests: one array of a row plan copied back (which: 0 slice offsets, 1 (length, sub-step) words, 2 position -> row, 3 / 4 sliced-ELL
 * column positions / values, 5 inverted diagonals, 6 right-hand-side scales, 7 sub-steps per slice, 8 row -> position, 9 level
 * extents); *bytes = its size, copied when it fits cap_bytes.  Row plans in column order are laid out on the device
 * (csrc/trisolve_build.hip); MI355X_TRISOLVE_BUILD=host in the environment keeps the host threads' route: the same arrays. */
int mi355x_trisolve_debug_get(mi355x_trisolve_plan_t plan, int which, void *out, size_t cap_bytes, size_t *bytes);
/* the same application over the same plans with one launch per dependency level and no hand-off between wavefronts (same
 * per-row order of the products: same bits): what a caller falls back to after a sync-free application gave up, whatever the
 * factor (ILU(0), ICC(0)); does not consult or change the abort flags; a sync-free application may follow */
int mi355x_trisolve_apply_levels(mi355x_handle_t h, mi355x_trisolve_plan_t lower, mi355x_trisolve_plan_t upper, const double *b, double *y);
/* development / tests: raise a plan's abort flag as a dependency wait that gave up would */
int mi355x_trisolve_debug_set_aborted(mi355x_trisolve_plan_t plan, int value);

/* ---- coarsening for smoothed aggregation (csrc/coarsen.hip; PCGAMG, harness/gamg.c) -------- */
/* Strength of connection over a square CSR matrix: for the stored entry t = (i, j)
 *   strong[t] = (j != i) && (fabs(a_t) > theta * sqrt(fabs(diag[i]) * fabs(diag[j])))
 * evaluated in double in exactly that order; a comparison with a NaN on either side is false, a zero diagonal entry makes every
 * nonzero off-diagonal entry of its row and column strong.  diag: what mi355x_csr_get_diagonal leaves (0 for a row without one).
 * One byte per stored entry, byte for byte the host twin's.  m == 0 launches nothing; m < 0 or a null array: hipErrorInvalidValue. */
int mi355x_csr_strength(mi355x_handle_t h, int m, const int *ai, const int *aj, const double *aa, const double *diag, double theta,
                        unsigned char *strong);
int mi355x_csr_strength_host(int m, const int *ai, const int *aj, const double *aa, const double *diag, double theta, unsigned char *strong);
/* Aggregation by a distance-2 maximal independent set of the undirected graph i ~ j <=> the stored entry (i, j) or (j, i) is strong
 * (the pattern need not be symmetric).  Node i's priority is the key (mix(i) >> 2) << 32 | i with the 32-bit finaliser
 * h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16.  The roots are the greedy set: nodes visited in decreasing
 * key, a node is a root iff no root lies within distance 2 (paths through non-roots count).  A root's aggregate number is its rank
 * among the roots in index order; a node with adjacent roots joins the one with the largest key, any other node the root with the
 * largest key among its neighbours' choices; a node without strong connections is its own root.  agg[i] in [0, *nagg).
 * The host twin is that loop.  The device entry runs rounds of two max-propagation steps (pull over a row, push with a 64-bit
 * atomicMax) and one decision step, the undecided count read once per round; *rounds = rounds taken, at most
 * mi355x_coarsen_round_cap() -- beyond it hipErrorNotReady and nothing is continued.  ai, aj, strong, agg: device arrays for the
 * device entry; nagg, rounds: host.  agg, *nagg equal the host twin's as integers.  m == 0 launches nothing. */
int mi355x_coarsen_mis2(mi355x_handle_t h, int m, const int *ai, const int *aj, const unsigned char *strong, int *agg, int *nagg, int *rounds);
int mi355x_coarsen_mis2_host(int m, const int *ai, const int *aj, const unsigned char *strong, int *agg, int *nagg);
int mi355x_coarsen_round_cap(void);

/* ---- halo pack / unpack (VecScatter) ---------------------------------- */
/* Pack_1    src/vec/vec/utils/vpscat.c:493   buf[k] = x[idx[k]] */
int mi355x_pack(mi355x_handle_t h, size_t n, const int *idx, const double *x, double *buf);
/* UnPack_1  src/vec/vec/utils/vpscat.c:503-534   INSERT: y[idx[k]] = buf[k]; ADD: y[idx[k]] += buf[k]; MAX: y[idx[k]] =
 * PetscMax(y[idx[k]], buf[k]) (idx == NULL means contiguous: y[k]).  ADD / MAX require idx entries to be distinct within one call. */
int mi355x_unpack_insert(mi355x_handle_t h, size_t n, const int *idx, const double *buf, double *y);
int mi355x_unpack_add(mi355x_handle_t h, size_t n, const int *idx, const double *buf, double *y);
int mi355x_unpack_max(mi355x_handle_t h, size_t n, const int *idx, const double *buf, double *y);

/* ---- measurement ------------------------------------------------------- */
/* STREAM-style copy (pattern: src/benchmarks/streams/CUDAVersion.cu) for the achievable-bandwidth line */
int mi355x_stream_triad(mi355x_handle_t h, size_t n, double alpha, const double *b, const double *c, double *a);

#ifdef __cplusplus
}
#endif
#endif
