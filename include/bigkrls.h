/*
 * bigkrls.h -- C ABI of libbigkrls_hip.so, the MI355X (gfx950) replacement for the
 * native numerics behind rdrr1990/bigKRLS's Rcpp boundary.
 *
 * Conventions (identical to the reference's bigmemory/Armadillo contract,
 * src/gauss_kernel.cpp:34-41 and every other BigMatrix wrapper):
 *   - every matrix is column-major float64, addressed as (ptr, nrow, ncol[, ld]);
 *   - the caller allocates every output; native code writes in place;
 *   - all sizes are int64_t; all functions return 0 on success or a BIGKRLS_E*
 *     code, with a human-readable message available from bigkrls_last_error().
 *
 * Two levels:
 *   Level 1  bigkrls_<op>()      host pointers in / host pointers out.  One entry
 *                                per .Call routine registered in the reference's
 *                                src/RcppExports.cpp:147-160.  Each stages its
 *                                operands through HBM, runs the HIP kernels and
 *                                copies the result back.
 *   Level 2  bigkrls_dev_<op>()  device pointers on an explicit bigkrls_ctx
 *                                (device + HIP stream + workspace).  N x N
 *                                objects stay in HBM (north_star: "bigmemory
 *                                file-backed N x N matrices are replaced by HIP
 *                                device buffers"); this is what the rewritten
 *                                bigKRLS()/predict()/crossvalidate() host code
 *                                calls.
 *
 * There is no CPU fallback: without a HIP device every compute entry point
 * returns BIGKRLS_ENODEVICE.
 *
 * Threading: a bigkrls_ctx (its stream, its look-ahead stream and its reusable
 * workspace) serves one host thread at a time -- the reference's native code is
 * single-threaded too (one PSOCK worker process per concurrent call,
 * R/bigKRLS.R:345-362); use one context per thread / per GPU. The Level-1 entry
 * points share one default context behind a mutex-protected creation and must not
 * be called concurrently. bigkrls_last_error() is per thread.
 * The eigensolver's persistent kernels spin on messages from other workgroups;
 * they are launched with grids no larger than the co-resident capacity of the
 * device and every wait is bounded: when a watchdog fires (the workgroups were not
 * co-resident, e.g. another process held part of the GPU) the decomposition is
 * redone in the same call with one launch per step -- never a hang. In
 * bigkrls_fit_dist the watchdog of ONE rank is agreed on by all ranks and the
 * partitioned decomposition is replayed once on every rank from a fresh copy of
 * its column block of K (csrc/fit.hip); BIGKRLS_EHIP (on every rank) only if the
 * replay fails too.
 * Verification: bigkrls_fit / bigkrls_fit_dist check EVERY decomposition -- the dense
 * path and the block Lanczos (Neig << N) alike -- against K itself before using it
 * (trace when the whole spectrum is known; all kept pairs through two fixed +-1
 * combinations: |K Q r - Q Lambda r| and | |Q r|^2 - k |; one pass over K) and redo
 * it once; a second failure is BIGKRLS_EHIP. (bigkrls_eigen with Neig << N checks the
 * last block of its Ritz pairs against K itself; inside a fit that sample is left to
 * the fit's check of all pairs in the first attempt and runs in a redo.) In a
 * multi-GPU fit every rank then runs
 * the lambda search on rank 0's eigenvalues (one broadcast of 8 Neig bytes): the
 * ranks' branch sequences cannot diverge. bigkrls_ctx_get_counters() says how often
 * a context took one of these paths.
 * Diagnostics: with BIGKRLS_TRACE_DIR=<dir> set, every process appends 64-bit hashes
 * of its collectives' inputs / outputs and of the fit's intermediate results to
 * <dir>/pid<pid>.trace (csrc/trace.hip; compared by tools/trace_diff.py). Off
 * otherwise (one environment lookup per process).
 */
#ifndef BIGKRLS_H
#define BIGKRLS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BIGKRLS_OK 0
#define BIGKRLS_EINVAL 1     /* bad argument (null pointer, negative size, ...)   */
#define BIGKRLS_ENODEVICE 2  /* no HIP device / device index out of range         */
#define BIGKRLS_EHIP 3       /* a HIP runtime call or kernel launch failed        */
#define BIGKRLS_ENOMEM 4     /* device allocation failed                          */
#define BIGKRLS_ENOCONV 5    /* an iterative numerical step did not converge      */

typedef struct bigkrls_ctx bigkrls_ctx;

/* ---- library / context ------------------------------------------------------ */
int bigkrls_version(void);
const char* bigkrls_last_error(void);
int bigkrls_device_count(int* count);

/* Create a context on `device` with its own non-blocking HIP stream. */
int bigkrls_ctx_create(int device, bigkrls_ctx** ctx);
/* Create a context that launches on an existing hipStream_t (e.g. the stream the
 * host framework already uses for these buffers). The stream is not owned. */
int bigkrls_ctx_create_on_stream(int device, void* hip_stream, bigkrls_ctx** ctx);
int bigkrls_ctx_destroy(bigkrls_ctx* ctx);
int bigkrls_ctx_sync(bigkrls_ctx* ctx);
void* bigkrls_ctx_stream(bigkrls_ctx* ctx);
/* Bytes of workspace currently held by the context (grown on demand, reused). */
int64_t bigkrls_ctx_workspace_bytes(bigkrls_ctx* ctx);
int bigkrls_ctx_release_workspace(bigkrls_ctx* ctx);

/* HIP-event sampling of the dominant kernels on their launch streams (used by
 * bench.py for the roofline figures; off by default). Names and their `work`:
 * "kernel_block" (flops 2*u*v*p), "band_av" (A22 V of a stage-1 panel, flops),
 * "band_update" / "band_update2" / "band_update4" (trailing update per panel at
 * k = 128 / the pieces of the two-panel update at k = 256 / the four-panel update at
 * k = 512, flops), "panel_qr" and "bulge_chase" (algorithmic bytes), "lanczos_kb" /
 * "lanczos_cgs2" (block-Lanczos step, flops), "symv" (one-stage path, bytes of the
 * lower triangle streamed), "solveforc_probe", "deriv_rows", "yhat_gemv" (algorithmic
 * bytes: 8 N K per probe, 8 N^2, 8 N^2), "vcov_syrk" (N (N + 1) K flops per matrix),
 * "kernel_loo_colsums" (u v n_cols exponentials), "kernel_loo_moments" (u v E exponentials, E per
 * row pair: one per chunk with a kind-0 or kind-1 entry plus one per kind-2 entry),
 * "kernel_loo_binsums" (u v n_cols exponentials), "deletion_residuals" (one call of
 * bigkrls_dev_deletion_residuals, 2 k sum_g m_g^2 flops over the units' sizes m_g). */
int bigkrls_ctx_set_profile(bigkrls_ctx* ctx, int enable);
int bigkrls_ctx_get_profile(bigkrls_ctx* ctx, const char* name, double* total_ms,
                            double* total_work, int64_t* launches);

/* How often this context took one of its recovery paths since it was created
 * (a GPU test session asserts all three are 0 outside its fault-injection cases):
 * out[0] decompositions redone because the fit's check against K failed,
 * out[1] decompositions replayed with launch-per-step kernels (a persistent kernel's
 *        watchdog, or ranks that kept different numbers of eigenpairs),
 * out[2] multi-GPU fits in which this rank's replicated eigenvalues differed from
 *        rank 0's (rank 0's are used by every rank: one broadcast of 8 Neig bytes). */
int bigkrls_ctx_get_counters(bigkrls_ctx* ctx, int64_t out[3]);

/* ---- device buffers (replaces bigmemory::big.matrix storage; reference type
 *      BigMatrix / SharedMemoryBigMatrix, e.g. src/gauss_kernel.cpp:34-35) ------ */
int bigkrls_dev_alloc(bigkrls_ctx* ctx, int64_t nbytes, void** dptr);
int bigkrls_dev_free(bigkrls_ctx* ctx, void* dptr);
int bigkrls_h2d(bigkrls_ctx* ctx, void* dst_dev, const void* src_host, int64_t nbytes);
int bigkrls_d2h(bigkrls_ctx* ctx, void* dst_host, const void* src_dev, int64_t nbytes);
int bigkrls_d2d(bigkrls_ctx* ctx, void* dst_dev, const void* src_dev, int64_t nbytes);
/* timing on the context's stream with HIP events (used by bench.py) */
int bigkrls_event_create(void** ev);
int bigkrls_event_destroy(void* ev);
int bigkrls_event_record(bigkrls_ctx* ctx, void* ev);
int bigkrls_event_elapsed_ms(void* ev_start, void* ev_stop, double* ms);

/* =============================================================================
 * Level 1: host-pointer drop-ins, one per reference .Call entry
 * ========================================================================== */

/* replaces BigGaussKernel(pA, pOut, sigma)            src/gauss_kernel.cpp:32-42
 * out[i,j] = exp(-sum_p (X[i,p]-X[j,p])^2 / sigma), n x n, diag == 1.
 * X need not be centred: the column means are subtracted on the device before the norms and products are taken. */
int bigkrls_gauss_kernel(const double* X, int64_t n, int64_t p, double sigma, double* out);

/* replaces BigTempKernel(pA, pB, pOut, sigma)         src/temp_kernel.cpp:32-44
 * out[i,j] = exp(-||A_i - B_j||^2 / sigma), A is u x p, B is v x p, out u x v.
 * A and B need not be centred: the column means of A are subtracted from both on the device. */
int bigkrls_temp_kernel(const double* A, int64_t u, const double* B, int64_t v, int64_t p,
                        double sigma, double* out);

/* replaces BigEigen(pA, Neig, pValBigMat, pVecBigMat) src/eigen.cpp:32-45
 * A symmetric n x n; vals[neig] descending; vecs n x neig (column k <-> vals[k]).
 * neig == n: full spectrum; neig < n: the neig ALGEBRAICALLY largest pairs.
 * Difference from the reference for neig < n: arma::eigs_sym (src/eigen.cpp:21, default form "lm") returns the
 * pairs of largest MAGNITUDE. The two agree on every positive semi-definite A -- a Gaussian kernel matrix, the only
 * thing bigKRLS passes (R/bigKRLS.R:266) -- and whenever |most negative eigenvalue| < the neig-th largest one; an
 * indefinite A whose negative end dominates gets different pairs here. A caller that needs "lm" on such a matrix
 * can call this on A and on -A and merge. */
int bigkrls_eigen(const double* A, int64_t n, int64_t neig, double* vals, double* vecs);

/* replaces BigSolveForc(pEigenvectors, Eigenvalues, y, lambda)  src/solveforc.cpp:67-78
 * Q is n x k; only vals[0..k) of the nvals passed are used (quirk Q1).
 * Outputs Le = sum_i (c_i/Ginv_ii)^2 and coeffs[n]. Q is left untouched. */
int bigkrls_solveforc(const double* Q, int64_t n, int64_t k, const double* vals, int64_t nvals,
                      const double* y, double lambda, double* Le, double* coeffs);

/* replaces BigMultDiag(pA, diag, pOut)                src/multdiag.cpp:26-37
 * out[:,i] = A[:,i]*diag[i], i < k (diag may be longer than k). */
int bigkrls_multdiag(const double* A, int64_t n, int64_t k, const double* diag, double* out);

/* replace BigCrossProd / BigXtX / BigTCrossProd / BigXXt   src/crossprod.cpp:18-85
 * crossprod : out (ak x bk) = A'B, A is n x ak, B is n x bk
 * xtx       : out (k x k)   = A'A
 * tcrossprod: out (an x bn) = A B', A is an x k, B is bn x k
 * xxt       : out (n x n)   = A A' */
int bigkrls_crossprod(const double* A, int64_t n, int64_t ak, const double* B, int64_t bk, double* out);
int bigkrls_xtx(const double* A, int64_t n, int64_t k, double* out);
int bigkrls_tcrossprod(const double* A, int64_t an, int64_t k, const double* B, int64_t bn, double* out);
int bigkrls_xxt(const double* A, int64_t n, int64_t k, double* out);

/* replaces BigDerivMat(pX, pK, pVCovMatC, pDerivatives, pVarAvgDerivatives, coeffs, sigma)
 *                                                     src/bigderiv_v3.cpp:113-132
 * X n x p (columns to differentiate), K n x n, V n x n, coeffs[n];
 * outputs D n x p and var[p]. Binary columns (exactly two distinct values) take
 * the first-difference branch (:31-87), the rest the continuous one (:90-106). */
int bigkrls_derivmat(const double* X, int64_t n, int64_t p, const double* K, const double* V,
                     double* D, double* var, const double* coeffs, double sigma);

/* replaces double BigNeffective(pX)                       src/Neffective.cpp:13-65, 67-76
 * X n x p; *neff = n (1 - 2 r / n^2) + 1 with r = sum_{i>j} |cor(row i, row j)|
 * (rows de-meaned and normalised). A constant row gives NaN, as in the reference. */
int bigkrls_neffective(const double* X, int64_t n, int64_t p, double* neff);

/* =============================================================================
 * Level 2: device-resident operators (all pointers are device pointers unless
 * the parameter name starts with h_)
 * ========================================================================== */

/* General kernel block: out[i,j] = exp(-||A_i - B_j||^2/sigma), out is u x v with
 * leading dimension ldo. If diag_shift >= 0, entries with i == j + diag_shift are
 * set to exactly 1 (column block [c0,c1) of the symmetric n x n kernel:
 * A = X, B = X + c0, diag_shift = c0). Pass diag_shift = -1 for predict.
 * A and B need not be centred: both are copied with the column means of A subtracted (extra device memory
 * O((u + v) p), no host synchronisation) before |a|^2 + |b|^2 - 2 a.b is formed; lda >= u, ldb >= v and ldo >= u, else
 * BIGKRLS_EINVAL. A block B
 * that lies inside A (same leading dimension) reads the copy of A, so every column block of one X sees the same rows. */
int bigkrls_dev_kernel_block(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda,
                             const double* B, int64_t v, int64_t ldb, int64_t p, double sigma,
                             double* out, int64_t ldo, int64_t diag_shift);

/* Fused kernel contraction: trans = 0: out (u x q, ldo) = K(A,B) W with W v x q (ldw);
 * trans = 1: out (v x q, ldo) = K(A,B)' W with W u x q (ldw). K(A,B) is exactly bigkrls_dev_kernel_block's
 * kernel with diag_shift = -1; it is rebuilt tile by tile in registers and never written to memory (extra
 * device memory O((u + v) (p + q)), never O(u v)). Deterministic: two calls give bitwise identical results.
 * A and B need not be centred (the column means of A are subtracted from both, as in bigkrls_dev_kernel_block). */
int bigkrls_dev_kernel_contract(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda,
                                const double* B, int64_t v, int64_t ldb, int64_t p, double sigma,
                                const double* W, int64_t q, int64_t ldw, int trans, double* out, int64_t ldo);

/* Grouped fused kernel contraction: out (v x G q, ldo >= v); the block of columns [g q, (g + 1) q) holds
 *   K(A[rows with h_group == g], B)' W[those rows],
 * i.e. what bigkrls_dev_kernel_contract(trans = 1) gives on the rows of one group, for all G groups in ONE launch.
 * K is exactly bigkrls_dev_kernel_block's kernel: the column means of ALL of A are subtracted from both operands.
 * A u x p (lda >= u), B v x p (ldb >= v), W u x q (ldw >= u) on the device; h_group (u labels in [0, G), any order) on
 * the host. The host sorts the labels (stable counting sort; rows that are not already grouped are gathered into a copy
 * of A and W in group order) and cuts every group into segments of loop rows: equal parts by the cost model of
 * bigkrls_dev_kernel_contract's split rule (rounds of resident waves x loop tiles per wave, over all groups together),
 * a part at least 16 loop tiles unless the group is smaller, the partial sums at most 64 MB. A wave takes 64 rows of
 * B, a chunk of 16 / 32 / 64 columns (any q) and one segment; a group of one segment is written straight into out,
 * the segments of a longer group are added by a second kernel in segment order: no atomics, the layout depends on the
 * group sizes only, two calls give bitwise identical results. An empty group gives zero columns. The u x v kernel is
 * never stored; extra device memory O(u (p + q)) plus the partials. A label outside [0, G) or G < 1 is BIGKRLS_EINVAL
 * naming the row. Profile name "kernel_contract_grouped", work 2 u v (p + q). */
int bigkrls_dev_kernel_contract_grouped(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda, const double* B,
                                        int64_t v, int64_t ldb, int64_t p, double sigma, const double* W, int64_t q,
                                        int64_t ldw, const int64_t* h_group, int64_t G, double* out, int64_t ldo);

/* Fused leave-one-column-out column sums: out (v x n_cols, ldo >= v),
 *   out[l, jj] = sum_i exp(-(||A_i - B_l||^2 - (A[i,c] - B[l,c])^2) / sigma),   c = h_cols[jj] (host, 0-based),
 * i.e. the column sums of bigkrls_dev_kernel_block's kernel K(A, B) with column c left out of the distance, for all
 * selected columns in one pass (A u x p, B v x p as in bigkrls_dev_kernel_contract; what n_cols calls of it with
 * trans = 1 and W = ones on copies of A and B without column c give, with the Gram tile shared between the columns).
 * The leave-out exponent is formed directly, never as K exp(+(A[i,c] - B[l,c])^2 / sigma). Extra device memory
 * O((u + v) (p + n_cols)), never O(u v). Deterministic: two calls give bitwise identical results. A and B need not
 * be centred. A column index outside [0, p) or n_cols < 1 is BIGKRLS_EINVAL. */
int bigkrls_dev_kernel_loo_colsums(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda, const double* B,
                                   int64_t v, int64_t ldb, int64_t p, double sigma, const int64_t* h_cols,
                                   int64_t n_cols, double* out, int64_t ldo);

/* Fused binned leave-one-column-out column sums: bigkrls_dev_kernel_loo_colsums' sums per bin of the left-out column.
 * h_labels (host, u x n_cols column-major) holds the bin of row i of A under selected column jj, an integer in
 * [0, h_nbins[jj]) -- every selected column groups the rows its own way, and a column may be selected more than once
 * with other labels. out (v x sum_jj h_nbins[jj], ldo >= v): the bins of column jj are consecutive columns, the
 * columns in the caller's order,
 *   out[l, off(jj) + b] = sum over i with h_labels[i, jj] = b of exp(-(||A_i - B_l||^2 - (A[i,c] - B[l,c])^2) / sigma),
 * c = h_cols[jj] (host, 0-based). One pass for all columns and bins: the rows of A are read in every column's bin order
 * through an index list (no gathered copies), long bins are cut into segments whose sums are added in a fixed order; an
 * empty bin gives zeros; at p = 1 the sums are exactly the bins' counts. Both operands are centred once, by the column
 * means of all of A. Extra device memory O((u + v) p + u n_cols + v sum nbins), never O(u v); no atomics; deterministic:
 * two calls give bitwise identical results. A column index outside [0, p), n_cols < 1, a column with fewer than 1 bin,
 * or a label outside its range (naming the row and the selected column) is BIGKRLS_EINVAL. Profile name
 * "kernel_loo_binsums". */
int bigkrls_dev_kernel_loo_binsums(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda, const double* B,
                                   int64_t v, int64_t ldb, int64_t p, double sigma, const int64_t* h_cols,
                                   int64_t n_cols, const int64_t* h_labels, const int64_t* h_nbins, double* out,
                                   int64_t ldo);

/* The weights of exact interventional Shapley values on the coefficients of a Gaussian-kernel fit. The p columns are
 * partitioned into M players: h_players (host) holds the player of column l, an integer in [0, M); NULL: one player per
 * column (M must equal p). Every player owns at least one column and M <= 128. Z (u x p) holds the explained rows,
 * X (n x p) the training rows, Bg (B x p) the background rows, all on the device, in the same units and PACKED: column-
 * major matrices of their own, a column every `rows` doubles (this entry takes no leading dimensions). For a
 * triple (r, b, i) player m has the factors A_m = exp(-sum_{l in m} (Z[r,l] - X[i,l])^2 / sigma) inside a coalition and
 * B_m = exp(-sum_{l in m} (Bg[b,l] - X[i,l])^2 / sigma) outside it, and
 *   W[r M + m, i] = (1/B) sum_b (A_m - B_m) sum_g w_g prod_{l != m} (B_l + t_g (A_l - B_l)),
 * (t_g, w_g) the Gauss-Legendre rule on [0,1] with ceil(M/2) nodes, which integrates the Shapley weights of this product
 * game exactly: W[r M + m, :] c is the Shapley value of player m for the function x -> sum_i c_i K(x, X_i) at Z[r,:],
 * its value function the mean over the background rows of the function at "Z[r,:] on the coalition's columns, the
 * background row elsewhere". W is (u M) x n, column-major and packed as well; its ROW ORDER is explained row by explained
 * row, the M players of a row adjacent (row r M + m), a training row per column. The products without player m are
 * prefix times suffix products, never quotients: factors that underflow to 0 give finite weights. A player whose columns
 * agree between Z[r,:] and every background row has the weight exactly 0.0. One thread per training row and a few
 * explained rows, the per-player arrays in registers for M <= 32 (buckets 8, 16, 20, 24, 32) and in LDS above (64, 128); the
 * background rows pass through LDS in chunks, so p <= 2048. Sums over the background rows and the nodes run in a fixed
 * order inside one thread: no atomics, no partial sums, and an entry depends on its own explained row, its training row
 * and the background only -- a row block of Z gives bitwise the rows of the whole call, and two calls give bitwise
 * identical results. Extra device memory: 4 p bytes. BIGKRLS_EINVAL naming the argument: a player index out of
 * range, a player without a column, M over the cap, B < 1. Profile name
 * "shapley_weights". */
int bigkrls_dev_shapley_weights(bigkrls_ctx* ctx, const double* Z, int64_t u, const double* X, int64_t n, const double* Bg,
                                int64_t B, int64_t p, double sigma, const int64_t* h_players, int64_t M, double* W);

/* Fused leave-out moments: out (v x n_entries, ldo >= v). h_entries (host) is 3 x n_entries column-major, entry e =
 * (kind, c, j) with 0-based columns, and with dc = A[i,c] - B[l,c], dj = A[i,j] - B[l,j], d2 = ||A_i - B_l||^2:
 *   out[l, e] = sum_i wgt exp(-max(d2 - dc^2 - [kind = 2] dj^2, 0) / sigma)
 *   kind 0: wgt = 1, j ignored (bigkrls_dev_kernel_loo_colsums' quantity);   kind 1: wgt = B[l,j] - A[i,j], j != c;
 *   kind 2: wgt = 1, columns c and j both left out of the distance, j != c.
 * One pass for all entries: the entries are sorted by c (stable) and those of one c share the Gram tile and
 * d2 - dc^2; the kind-0 and kind-1 entries of a chunk share ONE exponential (a kind-1 entry is one fused multiply-add
 * on it), a kind-2 entry takes its own. The exponents are formed directly, never as K exp(+dc^2 / sigma); the weight is
 * the difference of the centred copies of the operands, never B_j M0 - sum A_j e. An entry that leaves out every column
 * (kind 0 at p = 1, kind 2 at p = 2) gives exactly u. Results are in the caller's entry order. Extra device memory
 * O((u + v) (p + n_entries)), never O(u v); no atomics; deterministic: two calls give bitwise identical results. A and B
 * need not be centred. An unknown kind, a column outside [0, p), j = c for kinds 1 and 2, or n_entries < 1 is
 * BIGKRLS_EINVAL naming the entry. Profile name "kernel_loo_moments". */
int bigkrls_dev_kernel_loo_moments(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda, const double* B,
                                   int64_t v, int64_t ldb, int64_t p, double sigma, const int64_t* h_entries,
                                   int64_t n_entries, double* out, int64_t ldo);

/* Diagonal of a quadratic form: out[i] = sum_j (A V)[i,j] A[i,j] = diag(A V A')[i], A m x n (lda >= m),
 * V n x n (ldv >= n), both column-major; V is general (not assumed symmetric). out has m entries. The m x n product
 * is never stored (extra device memory: a few doubles per row and 128-column tile). Deterministic: two calls give
 * bitwise identical results. */
int bigkrls_dev_quadform_diag(bigkrls_ctx* ctx, int64_t m, int64_t n, const double* A, int64_t lda,
                              const double* V, int64_t ldv, double* out);

/* Weighted row sums of squares: out[i] = sum_j w[j] T[i,j]^2 = diag(T diag(w) T')[i], T m x k column-major
 * (ldt >= m), w (k) and out (m) on the device. With T = A Q and V = Q diag(w) Q' this is diag(A V A'), the quantity of
 * bigkrls_dev_quadform_diag, from the factors of V: 2 m n k flops for the product (bigkrls_dev_gemm) instead of
 * 2 m n^2, and with w >= 0 a sum without cancellation. One thread per row, the columns in order: deterministic, two
 * calls give bitwise identical results. k == 0 gives zeros; m == 0 does nothing. */
int bigkrls_dev_rowsumsq_weighted(bigkrls_ctx* ctx, int64_t m, int64_t k, const double* T, int64_t ldt,
                                  const double* w, double* out);

/* C (m x n) = alpha * op(A) op(B) + beta * C ; transa/transb: 0 = N, 1 = T. */
int bigkrls_dev_gemm(bigkrls_ctx* ctx, int transa, int transb, int64_t m, int64_t n, int64_t k,
                     double alpha, const double* A, int64_t lda, const double* B, int64_t ldb,
                     double beta, double* C, int64_t ldc);

/* Product with a modulated left operand: C (m x n, ldc >= m, overwritten) = (A o (r 1' + t s')) B, i.e.
 * C[i,j] = sum_l A[i,l] (r[i] + t[i] s[l]) B[l,j]; A m x k (lda >= m) and B k x n (ldb >= k) column-major and not
 * transposed, r and t (m) and s (k) on the device. The factor is applied to A in registers on its way to the
 * multiply; the modulated copy of A is never written (no extra device memory beside bigkrls_dev_gemm's split-K
 * partials). Tiles and split-K choice are bigkrls_dev_gemm's; deterministic, two calls give bitwise identical results,
 * and with r = 1, t = 0 the result is bitwise that of bigkrls_dev_gemm(0, 0, m, n, k, 1.0, A, lda, B, ldb, 0.0, C, ldc).
 * k == 0 gives zeros; m == 0 or n == 0 does nothing. */
int bigkrls_dev_gemm_modulated(bigkrls_ctx* ctx, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda,
                               const double* r, const double* t, const double* s, const double* B, int64_t ldb,
                               double* C, int64_t ldc);

/* Product with a doubly modulated left operand: C (m x n, ldc >= m, overwritten) = (A o F) B with
 *   F[i,l] = fma(fma(t1[i], s1[l], r1[i]), fma(t2[i], s2[l], r2[i]), d),
 * i.e. C[i,j] = sum_l A[i,l] ((r1[i] + t1[i] s1[l]) (r2[i] + t2[i] s2[l]) + d) B[l,j]; A m x k (lda >= m) and B k x n
 * (ldb >= k) column-major and not transposed, r1, t1, r2, t2 (m) and s1, s2 (k) on the device (s1 and s2 may be the
 * same vector), d a host scalar. The factor is applied to A in registers on its way to the multiply; the modulated copy
 * of A is never written (no extra device memory beside bigkrls_dev_gemm's split-K partials). What the two
 * bigkrls_dev_gemm_modulated calls it replaces -- against B and against diag(s1) B -- spend twice over, it spends once:
 * 2 m n k flops. Tiles and split-K choice are bigkrls_dev_gemm's; deterministic, two calls give bitwise identical
 * results; with r2 = 1, t2 = 0, d = 0 the result is bitwise that of bigkrls_dev_gemm_modulated(.., r1, t1, s1, ..), and
 * with r1 = 1, t1 = 0 as well that of bigkrls_dev_gemm(0, 0, m, n, k, 1.0, A, lda, B, ldb, 0.0, C, ldc).
 * k == 0 gives zeros; m == 0 or n == 0 does nothing. */
int bigkrls_dev_gemm_modulated2(bigkrls_ctx* ctx, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda,
                                const double* r1, const double* t1, const double* s1, const double* r2,
                                const double* t2, const double* s2, double d, const double* B, int64_t ldb, double* C,
                                int64_t ldc);

/* Weighted Gram matrix: M (k x k, ldm >= k, overwritten) = A' diag(omega) A, i.e. M[i,j] = sum_l omega[l] A[l,i] A[l,j];
 * A n x k column-major (lda >= n), omega (n) on the device. The weight is applied to one operand in registers on its way
 * to the multiply; no weighted copy of A is written. Only the 128 x 128 tiles on or below the diagonal are computed and
 * every entry with row >= column is stored at (i, j) and (j, i), inside diagonal tiles too: M[i,j] == M[j,i] bit for bit.
 * The contraction is split over n (bigkrls_dev_gemm's split rule over the computed tiles) and the slabs are added in a
 * fixed order: deterministic, two calls give bitwise identical results. Extra device memory: the slabs,
 * 8 s t 128^2 bytes for s splits and t computed tiles. k == 0 does nothing; n == 0 gives zeros. */
int bigkrls_dev_gram_weighted(bigkrls_ctx* ctx, int64_t n, int64_t k, const double* A, int64_t lda,
                              const double* omega, double* M, int64_t ldm);

/* Per-cluster score sums: S (k x G, lds >= k, overwritten), S[j,g] = sum over the rows i with h_cluster[i] == g of
 * e[i] A[i,j]; A n x k column-major (lda >= n) and e (n) on the device, h_cluster (n labels in [0, G), any order) on
 * the host. An empty cluster gives a zero column; a label outside [0, G) or G < 1 is BIGKRLS_EINVAL. The host sorts the
 * labels (stable counting sort, uploaded once; rows that are already grouped are read without the permutation), the
 * device adds every cluster's rows in an order that depends on the cluster sizes only: no floating-point atomics, two
 * calls give bitwise identical results. Extra device memory: 8 n + 8 pieces bytes of indices and 8 k doubles per piece of
 * a cluster that spans several 64-row chunks (at most n / 64 + G pieces). */
int bigkrls_dev_cluster_scores(bigkrls_ctx* ctx, int64_t n, int64_t k, const double* A, int64_t lda, const double* e,
                               const int64_t* h_cluster, int64_t G, double* S, int64_t lds);

/* Deletion residuals of a linear smoother H = Q diag(w) Q' (Q n x k column-major on the device, ldq >= n; h_w the k
 * weights on the host): for the rows S of every unit, d_et[S] = (I - H_SS)^-1 d_e[S] -- the residuals of the rows of S
 * under the fit without them, basis and weights held fixed. h_unit: n host labels in [0, G), any order (a label outside
 * is BIGKRLS_EINVAL naming the row; an empty unit is allowed); NULL: every row is its own unit, d_et = d_e / (1 - h) on
 * the leverages h_i = sum_j Q_ij^2 w_j (no solve; G is ignored). Units of one row take that formula with labels too,
 * bitwise the NULL call's values. route 0: a unit of 2 .. 256 rows is one workgroup of a fused kernel (gather of the
 * unit's rows, H_SS by the f64 MFMA, Cholesky and both triangular solves in place; four size classes, one launch each:
 * up to 16, 64 and 128 rows with I - H_SS in LDS, up to 256 rows with it in 514 KiB of workspace per unit, at most 128
 * units per launch), a larger one takes the general route: I - H_SS by bigkrls_dev_gemm, its eigenpairs by
 * bigkrls_dev_eigen, et_S = V diag(1 / theta) V' e_S; 8 m^2 bytes per unit, at most 2^30, else BIGKRLS_EINVAL naming the unit before anything is allocated. route 1: every unit of two rows or more takes
 * the general route. A pivot (smallest eigenvalue, leverage of a single row) that is not positive means a block
 * leverage of 1 or more: BIGKRLS_EINVAL naming the first such unit, its size and the pivot column; nothing is written
 * for that unit. d_hat (n, may be NULL): the leverages. d_S (k x G -- k x n without labels --, lds >= k, may be NULL):
 * the scores S[:, g] = Q_S' et_S, by bigkrls_dev_cluster_scores. Fixed summation orders, no floating-point atomics: two
 * calls give bitwise identical results. Profile name "deletion_residuals". */
int bigkrls_dev_deletion_residuals(bigkrls_ctx* ctx, int64_t n, int64_t k, const double* d_Q, int64_t ldq,
                                   const double* h_w, const double* d_e, const int64_t* h_unit, int64_t G, int32_t route,
                                   double* d_et, double* d_hat, double* d_S, int64_t lds);

/* out[:,i] = A[:,i]*diag[i] (diag on device). */
int bigkrls_dev_multdiag(bigkrls_ctx* ctx, const double* A, int64_t n, int64_t k, int64_t lda,
                         const double* diag, double* out, int64_t ldo);

/* Symmetric eigendecomposition, A (n x n, lda) is preserved.
 * vals[n_vals] receives the n_vals largest eigenvalues, descending (pass
 * n_vals = n for all of them, which the fit needs, quirk Q5);
 * vecs (n x n_vecs, ldv) receives the eigenvectors of the n_vecs largest.
 * If h_keep_thresh >= 0, n_vecs is determined on the device side as
 * lastkeeper = #{k : vals[k] >= h_keep_thresh * vals[0]} capped at n_vecs_max,
 * exactly bEigen's rule (R/bigKRLS_Rcpp_functions.R:190); *h_n_vecs returns it.
 *
 * Leading dimensions, for this entry and for bigkrls_dev_eigen_part, bigkrls_dev_eigen_implicit and
 * bigkrls_dev_eigen_auto: lda, ldx and ldv are ordinary column-major strides in doubles, each >= n (a shorter one is
 * BIGKRLS_EINVAL, named in the message, and nothing is launched or written). A, X and vecs may be blocks of larger
 * matrices: no alignment beyond that of a double (8 bytes) is required, only the n x n (A), n x p (X) block is read, and
 * nothing outside the n x n_vecs block of vecs is written (n_vecs = *h_n_vecs <= n_vecs_max; in the partition form the
 * other parts' columns are zeroed over their n rows only). */
int bigkrls_dev_eigen(bigkrls_ctx* ctx, const double* A, int64_t n, int64_t lda,
                      int64_t n_vals, double* vals,
                      int64_t n_vecs_max, double h_keep_thresh, double* vecs, int64_t ldv,
                      int64_t* h_n_vecs);

/* Multi-GPU variant (one process per GPU, the same A on every rank): everything up to and
 * including the divide & conquer is replicated, but only the slice
 * [n_vecs*part_index/part_count, n_vecs*(part_index+1)/part_count) of the kept eigenvector
 * columns is back-transformed; the other columns of vecs are returned as zeros, so that an
 * all-reduce (sum) of vecs over the ranks -- the RCCL exchange north_star names for the
 * eigenvector back-transform -- assembles Q exactly. part_count = 1 is bigkrls_dev_eigen. */
int bigkrls_dev_eigen_part(bigkrls_ctx* ctx, const double* A, int64_t n, int64_t lda,
                           int64_t n_vals, double* vals,
                           int64_t n_vecs_max, double h_keep_thresh, double* vecs, int64_t ldv,
                           int64_t* h_n_vecs, int32_t part_index, int32_t part_count);

/* The same for the Gaussian kernel matrix K(X, X) of X (device, n x p, ldx; bandwidth sigma) WITHOUT the matrix: block
 * Lanczos whose products K B_j are fused contractions (the kernel tile is rebuilt in registers, never stored). Needs
 * n >= 1024 and 4 n_vals <= n (BIGKRLS_EINVAL otherwise). There is no dense fallback: BIGKRLS_ENOCONV is returned. The
 * operator's diagonal is exp(-max(d2, 0) / sigma) with d2 at rounding level, not the exact 1 of bigkrls_dev_kernel_block. */
int bigkrls_dev_eigen_implicit(bigkrls_ctx* ctx, const double* X, int64_t n, int64_t ldx, int64_t p, double sigma,
                               int64_t n_vals, double* vals,
                               int64_t n_vecs_max, double h_keep_thresh, double* vecs, int64_t ldv,
                               int64_t* h_n_vecs);

/* Auto rank: the eigenpairs down to h_keep_thresh * lambda_1 (0 < h_keep_thresh <= 1 required) without a rank given.
 * A != NULL: the stored matrix A (n x n, lda; X, ldx, p, sigma are ignored). A == NULL: the Gaussian kernel of X as an
 * operator, as in bigkrls_dev_eigen_implicit. The block Lanczos grows its subspace until the Ritz values are resolved
 * down to the threshold: with c = #{theta_i >= h_keep_thresh theta_1} it stops when the first c + 1 pairs -- the kept
 * ones and one sentinel below the threshold -- have converged, and returns what a call with n_vals = c + 1 returns:
 * *h_n_vals = c + 1 values in vals, *h_n_vecs = c eigenvectors in vecs. n_vals_max is the cap: vals holds n_vals_max
 * doubles, vecs n_vals_max columns, and the workspace is that of a fixed run with n_vals = n_vals_max. More than
 * n_vals_max - 1 eigenvalues at or above the threshold: BIGKRLS_EINVAL, the message names the cap, the ratio
 * theta_cap / theta_1 reached and the threshold. Operator: n >= 1024 and 4 n_vals_max <= n, no dense fallback
 * (BIGKRLS_ENOCONV). Stored: the iteration is tried whenever n >= 1024 and 4 n_vals_max <= n; otherwise, and where it does
 * not converge, the dense path decomposes A with all values and the first c + 1 are returned. An eigenvalue whose
 * multiplicity exceeds the block size (128) can be missed, as with a given rank. */
int bigkrls_dev_eigen_auto(bigkrls_ctx* ctx, const double* A, int64_t n, int64_t lda, const double* X, int64_t ldx,
                           int64_t p, double sigma, double h_keep_thresh, int64_t n_vals_max, double* vals, double* vecs,
                           int64_t ldv, int64_t* h_n_vals, int64_t* h_n_vecs);

/* p[0 .. count) (device) = uniform values in [-0.5, 0.5) that depend on the element index and the seed only: the
 * start block of the block Lanczos, the same on every rank (seed 20240229 is the single-GPU library's). */
int bigkrls_dev_fill_random(bigkrls_ctx* ctx, double* p, int64_t count, uint32_t seed);
/* Orthonormalise the columns of the n x b block W (device, column-major, ld n; b <= 128) by Cholesky-QR applied
 * twice, in place; tmp: device scratch of the same size. h_R (host, b x b column-major) receives the upper
 * triangular R with W_in = W_out R, *h_breakdown is 1 when the Gram matrix was not positive definite (W is then
 * undefined); d_R (device, b x b, may be NULL) receives the same R. One step of the library's block Lanczos
 * (exposed for tests; the reference has no counterpart: its Neig < N branch is arma::eigs_sym,
 * src/eigen.cpp:18-22). */
int bigkrls_dev_cholqr2(bigkrls_ctx* ctx, double* W, double* tmp, int64_t n, int64_t b, double* h_R,
                        int32_t* h_breakdown, double* d_R);
/* One panel factorisation of the dense eigensolver's stage 1 (exposed for tests): the m x 64 panel P (device,
 * column-major, ld >= m; m >= 2) is factorised by the route the reduction takes for a panel of m rows under the current
 * BIGKRLS_PQ and BIGKRLS_S1_TPQ. 128 <= m <= 20 480: CholeskyQR2 + Householder reconstruction -- head, the Householder
 * kernel's slot, tail; the one-kernel form under BIGKRLS_PQ=fused; the Householder kernel alone under
 * BIGKRLS_PQ=householder. m < 128 (the last panels of a decomposition): the Householder kernel. m > 20 480,
 * BIGKRLS_PQ=steps or a context whose watchdog has fired: one launch per column. On return P holds R on and above the
 * diagonal of its top block and below it V (CholeskyQR2) or V's columns before their scaling, x_c = V[:, c] / scale_c with
 * the scales the reduction keeps beside tau (the Householder kernels and the per-column path); V (m x 64, ld m) the unit lower trapezoidal reflector block; T (64 x 64)
 * the upper triangular factor of H = I - V T V'; tau (64) its diagonal; Vw (m x 64, ld m) the operand W = V U of the
 * big product of stage 1 and Tfold (64 x 64) = U^-1 T, so that W Tfold = V T (Vw = V and Tfold = T wherever the split
 * form did not run, and for a panel CholeskyQR2 left to the Householder kernel, which alone *h_fallback = 1 reports).
 * m < 64: min(64, m) reflectors; columns m ... of V, entries m - 1 ... of tau and rows and columns m - 1 ... of T are
 * zero, and all of P is R. BIGKRLS_EINVAL: a null pointer, m < 2, ld < m, or -- where CholeskyQR2 would run, whose
 * kernels address the panel through 32-bit byte offsets -- 63 ld + m > 2^29. */
int bigkrls_dev_panel_factor(bigkrls_ctx* ctx, double* P, int64_t ld, int64_t m, double* Vw, double* V, double* T,
                             double* Tfold, double* tau, int32_t* h_fallback);
/* The symmetric rank-2k family of the MFMA GEMM core (exposed for tests): one unchanged call of the internal function
 * that `form` names. A and B are m x k (device, column-major, lda, ldb >= m), C is m x m (ldc >= m); with P = A B' the
 * update is C[i,j] += alpha P[i,j] for i >= j over a range of columns j, and the mirror forms store the new C[i,j] at
 * C[j,i] as well (i > j). Nothing else of C is written.
 *   form 0  syrk_lower: all columns, lower triangle only (the strict upper triangle is neither read nor written)
 *   form 1  syrk_mirror, 128-wide tiles: the 128-wide tile columns [begin, end) (end < 0 or too large: to the last)
 *   form 2  syrk_mirror, 64-wide tiles: the same columns; flags bit 0 (skip_first_column) leaves out the first 64
 *   form 3  syrk_mirror_cols: the 64-wide columns [begin, end) (begin < 0: 0; end < 0 or too large: to the last)
 *   form 4  syrk_mirror_set: C = alpha P on the lower triangle, mirrored; C is not read; needs k > 0
 * begin and end are ignored by forms 0 and 4; any other form or flag is BIGKRLS_EINVAL. */
int bigkrls_dev_syr2k(bigkrls_ctx* ctx, int form, int64_t m, int64_t k, double alpha, const double* A, int64_t lda,
                      const double* B, int64_t ldb, double* C, int64_t ldc, int64_t begin, int64_t end, int flags);
/* C (m x n, ldc; n <= 48) = A (m x k, lda) B (k x n, ldb), device pointers: gemm_nn_skinny48, the 128 x 48 tile of the
 * marginal-effects pass with its deterministic split-K (exposed for tests). m, n, k > 0. */
int bigkrls_dev_gemm_skinny48(bigkrls_ctx* ctx, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda,
                              const double* B, int64_t ldb, double* C, int64_t ldc);
/* n_batch independent products C_i (m_i x n_i, ldc_i) = A_i[:, kidx_i] B_i in one batched launch: gemm_batched_nn, the
 * merge products of the divide & conquer eigensolver (exposed for tests). Every argument is a host array of n_batch
 * entries; h_A, h_B, h_C and h_kidx hold device addresses as integers. A_i is m_i x k_i (lda_i) when h_kidx[i] == 0,
 * else column l of the operand is column kidx_i[l] of A_i (kidx_i: k_i 32-bit integers on the device); B_i is k_i x n_i.
 * max_m >= every m_i and max_n >= every n_i size the grid. The descriptors are uploaded as the eigensolver uploads
 * them; the call returns after the stream has been synchronised. */
int bigkrls_dev_gemm_batched(bigkrls_ctx* ctx, int64_t n_batch, const int64_t* h_m, const int64_t* h_n, const int64_t* h_k,
                             const int64_t* h_A, const int64_t* h_lda, const int64_t* h_B, const int64_t* h_ldb,
                             const int64_t* h_C, const int64_t* h_ldc, const int64_t* h_kidx, int64_t max_m, int64_t max_n);
/* d_T (device, m x m column-major, m = steps b) = the block-tridiagonal projected matrix of a block Lanczos run:
 * diagonal blocks 0.5 (A_j + A_j') from d_A_blocks (steps blocks of b x b), sub-diagonal blocks beta_{j+1} (upper
 * triangular) from d_beta_blocks (steps - 1 blocks are read), super-diagonal blocks their transposes. */
int bigkrls_dev_lanczos_projected(bigkrls_ctx* ctx, const double* d_A_blocks, const double* d_beta_blocks,
                                  int64_t steps, int64_t b, double* d_T);
/* dst (m x n, ldd) = src (m x n, lds), both on the device */
int bigkrls_dev_copy_matrix(bigkrls_ctx* ctx, const double* src, int64_t m, int64_t n, int64_t lds,
                            double* dst, int64_t ldd);

/* a = Q'y (k-vector), hoisted out of the lambda probes. Q rows [0,n), ld ldq >= n
 * (BIGKRLS_EINVAL otherwise, as in the two entries below). */
int bigkrls_dev_qty(bigkrls_ctx* ctx, const double* Q, int64_t n, int64_t k, int64_t ldq,
                    const double* y, double* a);

/* One solveforc probe on a row block of Q (n_rows x k, ldq): with
 * w_k = 1/(d_k+lambda): c_i = sum_k Q_ik w_k a_k, g_i = sum_k Q_ik^2 w_k,
 * *h_Le = sum_i (c_i/g_i)^2 over the block's rows. c (n_rows) may be NULL.
 * ldq >= n_rows. */
int bigkrls_dev_solveforc(bigkrls_ctx* ctx, const double* Q, int64_t n_rows, int64_t k, int64_t ldq,
                          const double* d, const double* a, double lambda,
                          double* c, double* h_Le);

/* Golden-section search exactly as bLambdaSearch (R/bigKRLS_Rcpp_functions.R:5-82)
 * on one device: h_vals_all[n_vals] are ALL eigenvalues (host copy, bounds loops,
 * quirk Q5); d (device) the first k of them. h_L/h_U < 0 mean "derive the bound".
 * Outputs lambda, the number of probes and (optionally) the probe trace
 * h_trace[2*max_trace] = (lambda_t, Le_t): the first min(probes, max_trace) pairs;
 * *h_nprobes is the full count. h_nprobes and h_trace may be NULL, h_vals_all may
 * be NULL when both bounds are given, h_tol <= 0 means 1e-3 n, ldq >= n. */
int bigkrls_dev_lambda_search(bigkrls_ctx* ctx, const double* Q, int64_t n, int64_t k, int64_t ldq,
                              const double* d, const double* a,
                              const double* h_vals_all, int64_t n_vals,
                              double h_L, double h_U, double h_tol,
                              double* h_lambda, int64_t* h_nprobes,
                              double* h_trace, int64_t max_trace);

/* Host-only helper: the U and L bounds of bLambdaSearch (:16-36). */
int bigkrls_lambda_bounds(const double* h_vals_all, int64_t n_vals, int64_t n,
                          double* h_L, double* h_U);

/* Row-block pass of the marginal-effects step (src/bigderiv_v3.cpp:13-111) in its
 * O(N^2) form. Krows is the block's rows of K stored as an n x n_rows column
 * block (K symmetric), X_full is n x p (all rows; the block is rows
 * [row0,row0+n_rows)), is_binary[p] int32 flags (host), c (n).
 * Outputs for the block: D (n_rows x p, ldd) and S (n_rows x p, lds) where S is
 * the vector whose V-quadratic form gives the variance (s for continuous
 * columns, KT_rs - KC_rs for binary ones). */
int bigkrls_dev_deriv_rows(bigkrls_ctx* ctx, const double* Krows, int64_t n, int64_t n_rows,
                           int64_t ldk, int64_t row0, const double* X_full, int64_t p, int64_t ldx,
                           const int32_t* h_is_binary, const double* c, double sigma,
                           double* D, int64_t ldd, double* S, int64_t lds);

/* var[j] = scale_j * sum_k wv_k (q_k' S[:,j])^2 with V = Q diag(wv) Q' never formed;
 * scale_j = 4/(sigma^2 n^2) (continuous) or 2 sd_j^2/n^2 (binary) is supplied by
 * the caller in h_scale[p]. h_var[p] on host. */
int bigkrls_dev_deriv_var(bigkrls_ctx* ctx, const double* Q, int64_t n, int64_t k, int64_t ldq,
                          const double* wv, const double* S, int64_t p, int64_t lds,
                          const double* h_scale, double* h_var);

/* small vector helpers used by the host layer (all on device) */
int bigkrls_dev_gemv(bigkrls_ctx* ctx, int trans, int64_t m, int64_t n, double alpha,
                     const double* A, int64_t lda, const double* x, double beta, double* y);
int bigkrls_dev_dot(bigkrls_ctx* ctx, int64_t n, const double* x, const double* y, double* h_out);
int bigkrls_dev_diag(bigkrls_ctx* ctx, const double* A, int64_t n, int64_t lda, double* out);
int bigkrls_dev_scale(bigkrls_ctx* ctx, int64_t n, double alpha, double* x);

/* device-resident BigNeffective: X n x p on device (leading dimension ldx), result on host */
int bigkrls_dev_neffective(bigkrls_ctx* ctx, const double* X, int64_t n, int64_t ldx, int64_t p,
                           double* h_neff);

/* =============================================================================
 * Level 2, whole-path entry points: the fit and the prediction as ONE call each, so that an R shim
 * is a single .Call and no N x N object crosses PCIe.
 * bigkrls_fit() is the numeric body of bigKRLS() (R/bigKRLS.R:175-470: validation, standardisation,
 * the five steps, rescaling); bigkrls_predict() that of predict.bigKRLS() (R/bigKRLS.R:590-621).
 * Following the reference's ownership rule, the caller allocates every output -- host arrays for the
 * small ones, device buffers for K / vcov.est.c / vcov.est.fitted -- and the library writes in place.
 * ========================================================================== */

typedef struct bigkrls_fit_options {
  int64_t struct_bytes;      /* sizeof(bigkrls_fit_options); checked                                  */
  double sigma;              /* <= 0: ncol(X)                                   R/bigKRLS.R:230     */
  double lambda;             /* <= 0: golden-section search                     :271-278            */
  double L, U;               /* < 0: derived bounds        R/bigKRLS_Rcpp_functions.R:16-36         */
  double eigtrunc;           /* < 0: 0.001 if n > 3000 else 0                   :195-201            */
  int64_t neig;              /* <= 0: n                                         :194                */
  int32_t derivative;        /* marginal effects (step 5)                       :321                */
  int32_t vcov_est;          /* variance matrices; derivative != 0 requires it  :239                */
  int32_t acf;               /* also BigNeffective(X), only when p > 2          :192, :412-416      */
  int32_t kernel_form;       /* 0: K stored (n x n on the device); 1: implicit -- K is never stored, every product
                                with it is a fused contraction that rebuilds its tiles from X. Implicit needs
                                neig > 0 with n >= 1024 and 4 neig <= n (block Lanczos, no dense fallback), one
                                GPU (bigkrls_fit only), d_K = d_vcov_c = d_vcov_fitted = NULL: the variance comes
                                as factors (d_vcov_q, vcov_w) or not at all. Other values: BIGKRLS_EINVAL          */
  const int64_t* which_derivatives;  /* 1-based like R; NULL: all columns       :206-215, :326      */
  int64_t n_which;
} bigkrls_fit_options;

typedef struct bigkrls_fit_outputs {
  int64_t struct_bytes;      /* sizeof(bigkrls_fit_outputs); checked */
  /* ---- caller-allocated host arrays; NULL = not wanted ---------------------------------------- */
  double* eigenvalues;       /* neig values (bigkrls_fit_auto: room for neig_max), descending; ALL are returned (quirk Q5) :268 */
  double* coeffs;            /* n                                                       :420         */
  double* yfitted;           /* n, original units                                       :428         */
  double* yfitted_std;       /* n, K c in standardised units                            :291         */
  double* derivatives;       /* n x pd column-major, rescaled incl. quirk Q6            :394-397     */
  double* derivatives_std;   /* n x pd, as BigDerivMat returns them                     :329         */
  double* avgderivatives;    /* pd                                                      :400         */
  double* var_avgderivatives;      /* pd                                                :403-407     */
  double* var_avgderivatives_std;  /* pd, before the rescaling                                        */
  int32_t* binaryindicator;  /* p flags: column has exactly two distinct values         :242         */
  double* lambda_trace;      /* 2 x max_trace: (lambda_t, Le_t) of every probe of the search          */
  int64_t max_trace;
  /* ---- caller-allocated DEVICE buffers, n x n column-major (ld = n); NULL = not returned ------- */
  double* d_K;               /* the kernel                                              :434         */
  double* d_vcov_c;          /* sd(y)^2 V                                               :438         */
  double* d_vcov_fitted;     /* sd(y)^2 V_yhat                                          :445         */
  /* ---- scalars written by the call ---------------------------------------------------------------- */
  int64_t lastkeeper;        /* kept eigenpairs        R/bigKRLS_Rcpp_functions.R:190                */
  int64_t neig;              /* length of `eigenvalues` */
  int64_t n_deriv;           /* pd: ncol of the derivative outputs */
  int64_t n_probes;          /* probes of the lambda search (0 when lambda was given) */
  double sigma, lambda;
  double Le, Looe;           /* leave-one-out loss, standardised and x sd(y)            :430         */
  double sigmasq;            /* ||y - yhat||^2 / n                                       :294         */
  double R2, R2AME;          /*                                                         :429, :392   */
  double Neffective;         /* n - sum_{all Neig} d/(d+lambda)                         :280         */
  double Neffective_acf;     /* NaN unless options.acf                                   :412-416     */
  double y_mean, y_sd;
  double phase_s[8];         /* HIP-event seconds: h2d, kernel, eigen, lambda, coeffs, vcov_c,
                                vcov_fitted, derivatives */
  /* ---- vcov.est.c as its factors: vcov.est.c = Q diag(w) Q' with Q the lastkeeper kept eigenvectors and
   *      w_j = sd(y)^2 sigmasq / (d_j + lambda)^2, the weights the fit itself uses (:299) in the units of d_vcov_c
   *      (:438). 8 n lastkeeper bytes instead of 8 n^2; everything after the fit can work from them
   *      (bigkrls_predict_factored, bigkrls_marginal_effects_factored). Requires options.vcov_est != 0; independent of
   *      d_vcov_c / d_vcov_fitted, which may be NULL (neither matrix nor its scratch is then formed). The factors are
   *      never truncated: if lastkeeper > vcov_q_cols_max the call returns BIGKRLS_EINVAL as soon as the decomposition
   *      is accepted, the message names both numbers and `lastkeeper` is set. In bigkrls_fit_dist every rank receives
   *      the whole n x lastkeeper Q (the eigenvectors are replicated there: no further exchange).
   *      vcov.est.fitted = Q diag(w_j d_j^2) Q' (:307 with K Q = Q D): its weights are formed by the host from
   *      `eigenvalues`. */
  double* d_vcov_q;          /* caller-allocated DEVICE buffer, n x vcov_q_cols_max, ld n; NULL = not wanted */
  int64_t vcov_q_cols_max;   /* its capacity in columns */
  double* vcov_w;            /* caller-allocated host array, vcov_q_cols_max doubles: receives w */
  int64_t vcov_q_cols;       /* written by the call: columns of Q / entries of w that are valid (= lastkeeper) */
} bigkrls_fit_outputs;

/* X is n x p column-major, y has n entries, both on the HOST (they are small: 8 n (p+1) bytes).
 * Errors of the reference's validation block (:183-240) come back as BIGKRLS_EINVAL with R's own
 * message text in bigkrls_last_error(). */
int bigkrls_fit(bigkrls_ctx* ctx, const double* h_X, const double* h_y, int64_t n, int64_t p,
                const bigkrls_fit_options* options, bigkrls_fit_outputs* out);

/* bigkrls_fit with the rank found by the fit (bigkrls_dev_eigen_auto) instead of given: options.neig is ignored, the
 * eigensolver keeps the pairs down to eigtrunc * lambda_1 and one value below it. Needs eigtrunc > 0 after the default
 * rule (n <= 3000 with eigtrunc unset, or eigtrunc = 0: BIGKRLS_EINVAL), n >= 1024 and 1 <= neig_max <= n / 4; there is
 * no multi-GPU form. neig_max is the cap of the rank search: outputs.eigenvalues must hold neig_max doubles (and
 * d_vcov_q, if wanted, at most neig_max - 1 columns are written), outputs.neig = lastkeeper + 1 is the number of values
 * written, and Neffective, the lambda bounds and the search use those values, as they use the `neig` values of a fit
 * with the rank given. More than neig_max - 1 eigenvalues at or above the threshold: BIGKRLS_EINVAL. The options and
 * outputs structs are those of bigkrls_fit, unchanged. */
int bigkrls_fit_auto(bigkrls_ctx* ctx, const double* h_X, const double* h_y, int64_t n, int64_t p,
                     const bigkrls_fit_options* options, int64_t neig_max, bigkrls_fit_outputs* outputs);

/* predict.bigKRLS (R/bigKRLS.R:590-621): newdata (u x p, host) is standardised with the TRAINING
 * means and sds, the u x n test kernel is built, predicted = K_new c sd(y) + mean(y).
 * With d_vcov_c (the fit's device-resident vcov.est.c) and h_se_pred or d_vcov_pred given, also
 * vcov.est.pred = var(y) K_new (vcov.est.c / var(y)) K_new' (:608), times sqrt(n / neffective) when
 * neffective > 0 (correct.SE, quirk Q10, :610-611), and se.pred = sqrt(diag) (:613).
 * d_newdataK (u x n) and d_vcov_pred (u x u) are optional caller-allocated device outputs. */
int bigkrls_predict(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                    const double* h_coeffs, double sigma, const double* h_newdata, int64_t u,
                    const double* d_vcov_c, double neffective,
                    double* h_predicted, double* h_se_pred, double* d_newdataK, double* d_vcov_pred);

/* predict.bigKRLS without the u x n and u x u matrices: the same inputs, validation, error messages and outputs as
 * bigkrls_predict (predicted, and se.pred when h_se_pred is given), for any number u of new points. The new points
 * are taken in row blocks of b: b is the largest multiple of 128 with 8 b n <= 2^30 bytes (the b x n test-kernel
 * block fits 1 GiB), at least 128, and min(b, u) rows are used when u is smaller (n = 20 000: b = 6 656). Per block:
 * the test kernel, its product with the coefficients, and with d_vcov_c the diagonal of K_b vcov.est.c K_b'
 * (bigkrls_dev_quadform_diag), times sqrt(n / neffective) when neffective > 0. Extra device memory:
 * O((u + n) p) plus the block and the quadratic form's partials, about 1.1 GiB at most, whatever u is. */
int bigkrls_predict_pointwise(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                              const double* h_coeffs, double sigma, const double* h_newdata, int64_t u,
                              const double* d_vcov_c, double neffective,
                              double* h_predicted, double* h_se_pred);

/* predict.bigKRLS from the factors of vcov.est.c (bigkrls_fit_outputs.d_vcov_q / vcov_w): d_Q is n x k on the device
 * (ldq >= n), h_w the k weights on the host, vcov.est.c = Q diag(w) Q'. Validation, standardisation, error messages and
 * the sqrt(n / neffective) factor are those of bigkrls_predict; d_Q NULL is "no vcov.est.c".
 * With d_newdataK and d_vcov_pred both NULL it is the counterpart of bigkrls_predict_pointwise: row blocks of b new
 * points, b the largest multiple of 128 with 8 b (n + k) <= 2^30 bytes (the b x n test-kernel block AND its b x k
 * product with Q fit 1 GiB together), at least 128, min(b, u) rows when u is smaller (n = 20 000, k = 250:
 * b = 6 528). Per block: the test kernel, its product with the coefficients, T = K_b Q (bigkrls_dev_gemm) and
 * se^2_i = sum_j w_j T_ij^2 (bigkrls_dev_rowsumsq_weighted): 2 b n k flops where bigkrls_predict_pointwise spends
 * 2 b n^2. Extra device memory: 8 b (n + k) <= 2^30 bytes for the block and T, 8 s b k bytes for the split-K partials
 * of the product (s is the split count bigkrls_dev_gemm chooses for a b x k result: a handful while the tiles of T
 * leave the GPU partly idle, 1 once they fill it, so the partials shrink relative to T as k grows) and
 * 8 ((n + b) (2 p + 1) + 2 u + k) bytes of vectors and operand copies. n = 20 000, p = 20, k = 250 (b = 6 528,
 * s <= 5): below 1.25 GiB for u up to millions of points.
 * With d_newdataK (u x n) or d_vcov_pred (u x u) given it is the counterpart of bigkrls_predict: the whole test
 * kernel, T = K_new Q (u x k), vcov.est.pred = (T diag(w)) T' and its diagonal from bigkrls_dev_rowsumsq_weighted;
 * extra device memory 8 u (2 k + p) bytes beside the outputs (and 8 u n when d_newdataK is NULL). */
int bigkrls_predict_factored(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                             const double* h_coeffs, double sigma, const double* h_newdata, int64_t u,
                             const double* d_Q, int64_t ldq, int64_t k, const double* h_w, double neffective,
                             double* h_predicted, double* h_se_pred, double* d_newdataK, double* d_vcov_pred);

/* Marginal effects of a fitted model at new data points (no counterpart in the reference, which computes them at
 * the training rows only, R/bigKRLS.R:318-407). X (n x p), y, coeffs (n) and sigma are the fit's; newdata (u x p,
 * host) is standardised with the TRAINING means and sds. h_which (1-based, n_which entries) selects the columns J;
 * NULL: all p. Binary training columns (exactly two distinct values) take the first difference between the two
 * training values; newdata must hold one of those two values in such a column (else BIGKRLS_EINVAL naming it).
 * Outputs in the original units, like the fit's: h_derivatives (u x |J| column-major; may be NULL), h_avg (|J|), and,
 * with d_vcov_c (the fit's n x n device-resident vcov.est.c, ld n) given, h_var (|J|) = the variance of each average;
 * d_vcov_c NULL requires h_var NULL. With newdata = X the results equal the fit's derivatives, avgderivatives and
 * var.avgderivatives. The u x n test kernel is never formed (bigkrls_dev_kernel_contract). */
int bigkrls_marginal_effects(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                             const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                             const double* h_newdata, int64_t u, const double* d_vcov_c, double* h_derivatives,
                             double* h_avg, double* h_var);

/* bigkrls_marginal_effects with vcov.est.c given by its factors (d_Q n x k on the device, ldq >= n; h_w the k weights
 * on the host) in place of d_vcov_c: everything up to the variance step is shared, and that step is the fit's own
 * var_j = scale_j sum_k w_k (q_k' s_j)^2 (bigkrls_dev_deriv_var) instead of the product vcov.est.c S and column
 * dots: 2 n k |J| flops instead of 2 n^2 |J|. d_Q NULL requires h_var NULL. */
int bigkrls_marginal_effects_factored(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                      const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                                      const double* h_newdata, int64_t u, const double* d_Q, int64_t ldq, int64_t k,
                                      const double* h_w, double* h_derivatives, double* h_avg, double* h_var);

/* Pointwise standard errors of the marginal effects: h_se (u x |J| column-major, the column order of h_derivatives)
 * = the standard error of every derivative bigkrls_marginal_effects returns for the same inputs, in the original
 * units. Validation, standardisation, binary detection and error messages are bigkrls_marginal_effects'. vcov.est.c
 * comes as the n x n matrix (d_vcov_c, ld n) or as its factors (d_Q n x k, ldq >= n, on the device; h_w the k weights
 * on the host): exactly one of d_vcov_c and d_Q is given, else BIGKRLS_EINVAL.
 * In standardised units D[i,j] = g_ij' c with g_ij[l] = Kn[i,l] (r_i + t_i s_l) (continuous j: s = Xs[:,j],
 * r_i = -(2/sigma) Zs_ij, t_i = 2/sigma; binary j: s = the training group indicator and r_i, t_i the two weights of
 * the first difference for the group of new point i), so Var(D[i,j]) = g_ij' V g_ij and
 *   se[i,j] = sqrt(f_j sum_m w_m ((G_j Q)[i,m])^2) / sd(x_j),   G_j = Kn o (r 1' + t s'),
 * with f_j = 2 for binary columns (the reference's factor, src/bigderiv_v3.cpp:85, as in var.avgderivatives) and 1
 * otherwise. With u = 1, se[0,j]^2 equals bigkrls_marginal_effects' h_var[j] for every column.
 * The new points are taken in row blocks of b. From the factors b is bigkrls_predict_factored's: the largest multiple
 * of 128 with 8 b (n + k) <= 2^30 bytes, at least 128; per block the test kernel once, and per column
 * T = G_j Q (bigkrls_dev_gemm_modulated: G_j is never stored) and bigkrls_dev_rowsumsq_weighted: 2 u n k flops per
 * column. From the matrix (the compatibility path) b is the largest multiple of 128 with 16 b n <= 2^30 bytes, at
 * least 128; G_j is written beside the block and bigkrls_dev_quadform_diag gives the diagonal: 2 u n^2 flops per column,
 * n / k times the factors' -- the factors are the fast form. block_rows = 0 chooses b as above; another value overrides
 * it and must be a positive multiple of 128 (BIGKRLS_EINVAL otherwise). Every row's result is bitwise independent of b
 * while the products take one k split (n < 1024); beyond that the split count follows the block's shape, as in
 * bigkrls_dev_gemm, and blockings agree to rounding. Two calls with the same b are bitwise identical.
 * Extra device memory: the block and T (or G_j), at most 1 GiB; the products' split partials; and
 * 8 ((u + n) (p + 2 |J|) + u |J| + k) bytes of vectors -- independent of u beyond O(u (p + |J|)). */
int bigkrls_marginal_effects_se(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                                const double* h_newdata, int64_t u, const double* d_vcov_c, const double* d_Q,
                                int64_t ldq, int64_t k, const double* h_w, int64_t block_rows, double* h_se);

/* Interaction effects of a fitted model at new data points: does the effect of x_j depend on x_k? (No counterpart in
 * the reference.) X, y, coeffs, sigma, newdata and u as in bigkrls_marginal_effects. h_pairs holds m pairs of 1-based
 * column indices, column-major (pair i is h_pairs[2 i], h_pairs[2 i + 1]); a pair is taken ordered (j <= k), and output
 * column i belongs to pair i. In standardised units, with the first-order modulation m_j(i,l) = r_j[i] + t_j[i] s_j[l] of
 * bigkrls_marginal_effects_se (continuous j: s = Xs[:,j], r = -(2/sigma) Zs[:,j], t = 2/sigma; binary j: s the training
 * group indicator, r and t the two first-difference weights), the Gaussian kernel factorises over the columns and
 *   G_jk = Kn o m_j o m_k - (2/sigma) delta_jk Kn,      I[i,(j,k)] = G_jk[i,:] c:
 * continuous x continuous the cross-derivative d^2 yhat / dx_j dx_k (j = k: the second derivative), binary x continuous
 * the derivative in x_k of the first difference in x_j, binary x binary (j != k) the second difference
 * (yhat_11 - yhat_10 - yhat_01 + yhat_00) / ((z1 - z0)_j (z1 - z0)_k). Original units: times sd(y) / (sd(x_j) sd(x_k)).
 * Outputs: h_interactions (u x m column-major; may be NULL), h_avg (m) the column means, and h_var (m) the variance of
 * each mean, a'V a with a = (1/u) 1'G_jk, times f_jk = 2 when a column of the pair is binary (the reference's factor,
 * src/bigderiv_v3.cpp:85, applied once) and 1 otherwise. vcov.est.c comes as the n x n matrix (d_vcov_c, ld n) or as
 * its factors (d_Q n x k on the device, ldq >= n; h_w the k weights on the host), at most one of them; with neither,
 * h_var must be NULL. Validation and its messages are bigkrls_marginal_effects' (finite newdata, binary columns of a
 * pair hold one of the two training values, constant training column); in addition a pair index outside [1, p], a pair
 * (j, j) on a binary column and a pair given twice (after ordering) are BIGKRLS_EINVAL, each naming the pair.
 * The u x n test kernel is never formed: two bigkrls_dev_kernel_contract calls of width q = 1 + |J'| + m (J' the columns
 * that occur in a pair) and a per-row finalise each. Extra device memory: O((u + n)(p + q)) and the contractions'
 * partials. */
int bigkrls_interaction_effects(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                const double* h_coeffs, double sigma, const int64_t* h_pairs, int64_t m,
                                const double* h_newdata, int64_t u, const double* d_vcov_c, const double* d_Q,
                                int64_t ldq, int64_t k, const double* h_w, double* h_interactions, double* h_avg,
                                double* h_var);

/* Pointwise standard errors of the interaction effects: h_se (u x m column-major, the columns of h_interactions) with
 *   Var(I[i,(j,k)]) = G_jk[i,:] V G_jk[i,:]',      se = sqrt(f_jk Var) sd(y) / (sd(x_j) sd(x_k)),
 * G_jk, f_jk, pairs, validation and messages as bigkrls_interaction_effects; exactly one of d_vcov_c and d_Q is given
 * (else BIGKRLS_EINVAL). With u = 1, se[0,i]^2 equals bigkrls_interaction_effects' h_var[i] for every pair. The new
 * points are taken in row blocks by bigkrls_marginal_effects_se's rules (from the factors 8 b (n + k) <= 2^30 bytes,
 * from the matrix 16 b n <= 2^30, b a multiple of 128 and at least 128; block_rows = 0, or a positive multiple of 128
 * that overrides b). Per block the test kernel once; per pair, from the factors T = G_jk Q
 * (bigkrls_dev_gemm_modulated2: G_jk is never stored) and bigkrls_dev_rowsumsq_weighted, 2 u n k flops per pair; from
 * the matrix (the compatibility path) G_jk is written beside the block, with the same fma expression, and
 * bigkrls_dev_quadform_diag gives the diagonal. Every row's result is bitwise independent of b while the products take
 * one k split (n < 1024); two calls with the same b are bitwise identical. */
int bigkrls_interaction_effects_se(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                   const double* h_coeffs, double sigma, const int64_t* h_pairs, int64_t m,
                                   const double* h_newdata, int64_t u, const double* d_vcov_c, const double* d_Q,
                                   int64_t ldq, int64_t k, const double* h_w, int64_t block_rows, double* h_se);

/* Partial dependence of the fitted outcome on one predictor at a time, with its covariance over the grid (no
 * counterpart in the reference). For every selected column j (h_which, 1-based, n_which entries; NULL: all p) and every
 * raw grid value v of it (h_grid: the columns' grids concatenated, column jj's at h_grid_off[jj] .. h_grid_off[jj + 1],
 * G_j >= 1 values each; T = h_grid_off[n_which] in all):
 *   h_pd  = the mean over the reference rows of the prediction with column j set to v (original units),
 *   h_se  = its standard error (T values; may be NULL),
 *   h_cov = the G_j x G_j covariance of column j's curve, column-major, the columns' blocks one after the other
 *           (sum_j G_j^2 doubles; may be NULL).
 * The reference rows are h_newdata (u x p, host), standardised with the TRAINING means and sds; NULL: the training rows
 * (u is then ignored). Column j of the reference rows is never read for column j's curve. Standardisation, validation
 * and error messages follow bigkrls_marginal_effects. vcov.est.c comes as the n x n matrix (d_vcov_c, ld n) or as its
 * factors (d_Q n x k on the device, ldq >= n; h_w the k weights on the host): at most one of them (else BIGKRLS_EINVAL);
 * with neither, h_se and h_cov must be NULL. The variances carry bigkrls_predict's factor for neffective > 0, so with
 * the same neffective h_se^2 is the mean of bigkrls_predict's vcov.est.pred over the rewritten rows.
 * The Gaussian kernel factorises over the columns, so in standardised units pd_j(v) = mean(y) + sd(y) a_j(v)' c with
 * a_j(v)[l] = (1/u) M[l,j] exp(-(vs - Xs[l,j])^2 / sigma) and M = bigkrls_dev_kernel_loo_colsums(Zs, Xs): ONE fused
 * O(u n) pass for all columns; per column A_j (G_j x n) is written, pd = A_j c, and cov_j = (A_j Q diag(w)) (A_j Q)' or
 * (A_j vcov.est.c) A_j', its diagonal from bigkrls_dev_rowsumsq_weighted or bigkrls_dev_quadform_diag.
 * 8 G_j n <= 2^30 bytes (A_j fits 1 GiB unblocked), else BIGKRLS_EINVAL naming the column, G_j and the cap. */
int bigkrls_partial_dependence(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                               const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                               const double* h_newdata, int64_t u, const double* h_grid, const int64_t* h_grid_off,
                               const double* d_vcov_c, const double* d_Q, int64_t ldq, int64_t k, const double* h_w,
                               double neffective, double* h_pd, double* h_se, double* h_cov);

/* Accumulated local effects (Apley & Zhu): the ALE curve of the fitted outcome on one predictor at a time, with its
 * covariance over the bin edges (no counterpart in the reference). Arguments as bigkrls_partial_dependence, with h_grid
 * holding the raw bin EDGES z_0 < z_1 < ... < z_B of every selected column (column i's at h_grid_off[i] ..
 * h_grid_off[i + 1], G_i = B_i + 1 >= 2 values). Reference row i falls into bin b(i) = the smallest b >= 1 with
 * Z[i,j] <= z_b (a row equal to z_0 goes to bin 1), n_b rows per bin. In standardised units, with
 * M_j = bigkrls_dev_kernel_loo_binsums(Zs, Xs) (ONE fused O(u n) pass for all columns and bins) and
 * phi_j(v, l) = exp(-(vs - Xs[l,j])^2 / sigma):
 *   D_j[b,l]  = M_j[l,b] (phi_j(z_b, l) - phi_j(z_{b-1}, l)) / n_b          the local effect of bin b is sd(y) D_j[b,:] c
 *   g(z_k)    = sum_{b <= k} local_b, g(z_0) = 0
 *   ale_j(z_k) = g(z_k) - (1/u) sum_b n_b (g(z_{b-1}) + g(z_b)) / 2          (ALEPlot's centring)
 * so ale_j = sd(y) A_j c with A_j (G_j x n) written by one elementwise kernel, and cov_j = f A_j vcov.est.c A_j' from
 * either form of vcov.est.c, f bigkrls_predict's factor for neffective > 0:
 *   h_ale = the curve at the edges (T = h_grid_off[n_which] values, original units of y, centred: no mean(y) is added),
 *   h_se  = its standard errors (T values; may be NULL),   h_cov = the G_i x G_i blocks (may be NULL).
 * BIGKRLS_EINVAL naming the column (and bin): fewer than 2 edges, edges that are not finite or not strictly increasing, a
 * reference value outside [z_0, z_B], an empty bin, more than the cap 8 G_i n <= 2^30 bytes allows. */
int bigkrls_accumulated_effects(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                                const double* h_newdata, int64_t u, const double* h_edges, const int64_t* h_grid_off,
                                const double* d_vcov_c, const double* d_Q, int64_t ldq, int64_t k, const double* h_w,
                                double neffective, double* h_ale, double* h_se, double* h_cov);

/* Shapley effects: how much of one row's prediction is due to each predictor -- exact interventional Shapley values of
 * the fitted prediction, with standard errors (no counterpart in the reference).
 * Players: the columns of X are partitioned into M players, h_players[l] in {0 .. M-1} the player of column l (host, p
 * labels; NULL: one player per column, M = p); every player owns at least one column, M <= 128. Grouping makes a set of
 * dummies count as one feature.
 * Value function: against the background sample h_background (B x p, host, column-major),
 *   v(S; x) = (1/B) sum_b f(x on the columns of the players in S, b elsewhere),
 * f the fitted prediction in original units; all rows are standardised with the TRAINING means and sds, as
 * bigkrls_predict does. The explained rows are h_newdata (u x p); NULL: the training rows (u is then ignored).
 * Result: with A_m / B_m the factors of bigkrls_dev_shapley_weights in standardised units,
 *   phi_m(x_r) = (sd(y)/B) sum_b sum_i c_i (A_m - B_m) sum_g w_g prod_{l != m} (B_l + t_g (A_l - B_l)) = sd(y) W[r M + m, :] c
 *   h_phi      = phi, u x M with the players of a row adjacent (h_phi[r M + m]), original units of y,
 *   h_baseline = the mean over b of bigkrls_predict at the background rows (one value),
 *   h_se       = the standard errors of phi in h_phi's order (may be NULL).
 * Efficiency: sum_m phi_m(x_r) = bigkrls_predict(x_r) - baseline.
 * Variance: Var phi_m(x_r) = f sd(y)^2 W[r M + m, :] V W[r M + m, :]' with V = vcov.est.c / sd(y)^2, the covariance of the
 * coefficients in standardised units -- d_vcov_c and the factors are the fit's vcov.est.c itself, which carries sd(y)^2 --
 * and f bigkrls_predict's factor for neffective > 0 (the correct_SE convention of bigkrls_partial_dependence). It is
 * conditional on X and on the background rows. vcov.est.c comes as the n x n matrix or as its factors, at most one of
 * them (else BIGKRLS_EINVAL); with neither, h_se must be NULL. The kernel matrix is never needed.
 * The explained rows are taken in blocks of b rows: the largest b with 8 b M n <= 2^30 bytes, at least 1; block_rows > 0
 * overrides it. Per block: bigkrls_dev_shapley_weights, phi = W c (bigkrls_dev_gemv), and T = W Q
 * (bigkrls_dev_gemm) with bigkrls_dev_rowsumsq_weighted, or bigkrls_dev_quadform_diag from the matrix. Every entry of W
 * is bitwise independent of b. h_phi and h_se of a row are bitwise independent of b as long as the products split alike
 * for both block shapes (bigkrls_dev_gemv's column splits, bigkrls_dev_gemm's k splits: one each for n <= 64), and agree
 * to rounding otherwise. Two calls with the same b are bitwise identical.
 * BIGKRLS_EINVAL naming the argument: a player index out of range, an empty player, M over the cap of 128, B < 1,
 * newdata or background with missing or infinite values, p > 2048. Extra device memory: the block and T, and
 * 8 ((n + u + B) p + n + k + 2 u M + B) bytes of vectors. */
int bigkrls_shapley_effects(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                            const double* h_coeffs, double sigma, const int64_t* h_players, int64_t M,
                            const double* h_newdata, int64_t u, const double* h_background, int64_t B,
                            const double* d_vcov_c, const double* d_Q, int64_t ldq, int64_t k, const double* h_w,
                            double neffective, int64_t block_rows, double* h_phi, double* h_se, double* h_baseline);

/* Conditional effects: the marginal effect of x_j along a moderator x_k, with its covariance over the grid (no
 * counterpart in the reference). h_pairs is 2 x m column-major, 1-based: pair i = (effect j, moderator k). For every pair
 * and every raw grid value v of x_k (h_grid: the pairs' grids concatenated, pair i's at h_grid_off[i] .. h_grid_off[i + 1],
 * G_i >= 1 values each; T = h_grid_off[m] in all):
 *   h_ce  = the mean over the reference rows of the marginal effect of x_j with column k set to v (original units):
 *           the derivative for a continuous j (k = j: the slope of the partial-dependence curve), the first difference
 *           between its two training values over their gap for a binary j,
 *   h_se  = its standard error (T values; may be NULL),
 *   h_cov = the G_i x G_i covariance of pair i's curve, column-major, the pairs' blocks one after the other
 *           (sum_i G_i^2 doubles; may be NULL).
 * They are avgderivatives and var.avgderivatives of bigkrls_marginal_effects on the reference rows with column k set to
 * v, in its units and with its factor 2 on the variances of a binary j. Reference rows, grids, value and covariance
 * layouts, the forms of vcov.est.c and the cap 8 G_i n <= 2^30 bytes are bigkrls_partial_dependence's, per pair instead of
 * per column; column k of the reference rows is never read, nor column j for a binary j. BIGKRLS_EINVAL naming the pair:
 * a pair (j, j) on a binary column, a pair given twice, an index outside [1, p], a grid value of a binary moderator
 * that is not one of its two training values, a grid above the cap.
 * In standardised units CE_jk(v) = a_jk(v)' c with a_jk(v)[l] = E_k(v)[l] times a moment of the test kernel with column
 * k left out (csrc/condeff.hip): ONE fused O(u n) pass bigkrls_dev_kernel_loo_moments(Zs, Xs) for all pairs (kind 1 for
 * a continuous j != k, kind 0 for j = k, kind 2 for a binary j; deduplicated); per pair A_jk (G_i x n) is written and the
 * values, variances and covariance come from bigkrls_partial_dependence's tail. */
int bigkrls_conditional_effects(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                const double* h_coeffs, double sigma, const int64_t* h_pairs, int64_t m,
                                const double* h_newdata, int64_t u, const double* h_grid, const int64_t* h_grid_off,
                                const double* d_vcov_c, const double* d_Q, int64_t ldq, int64_t k, const double* h_w,
                                double* h_ce, double* h_se, double* h_cov);

/* Average marginal effects by subgroup with their joint covariance (no counterpart in the reference). X, y, coeffs,
 * sigma, h_which, newdata and u as in bigkrls_marginal_effects (validation, standardisation, binary columns and error
 * messages are its own); h_group holds u labels in [0, G) (host, any order; a label outside, or G < 1, is BIGKRLS_EINVAL
 * naming the row). Outputs, original units:
 *   h_derivatives (u x |J| column-major; may be NULL): the pointwise effects, bigkrls_marginal_effects',
 *   h_ame (G x |J| column-major): ame[g, jj] = the mean of column jj of the derivatives over the rows of group g (an
 *         empty group: NaN),
 *   h_cov ((G |J|) x (G |J|) column-major, entry index e = jj G + g: the groups of one variable are adjacent): the joint
 *         covariance of all of them. Written exactly when vcov.est.c is given -- as the n x n matrix (d_vcov_c, ld n)
 *         or as its factors (d_Q n x k on the device, ldq >= n; h_w the k weights on the host), at most one of the two;
 *         with neither h_cov must be NULL.
 * In standardised units ame_e = sd(y) a_e S_e' c, where S_e (n) is bigkrls_marginal_effects' column-side vector s / a of
 * variable jj over the rows of group g, and a_e = -(2 / sigma) / (n_g sd(x_j)) for a continuous column,
 * +1 / ((z1 - z0) n_g sd(x_j)) for a binary one. cov[e, f] = a_e a_f S_e' V S_f with V = vcov.est.c (sd(y) cancels), and
 * a binary entry carries a further sqrt(2) -- the reference's factor 2 on the variance (src/bigderiv_v3.cpp:85), one
 * square root per side -- so that every diagonal entry is bigkrls_marginal_effects' h_var on the group's rows and the
 * matrix stays positive semi-definite. The rows and columns of an empty group are zero.
 * The row side is bigkrls_marginal_effects' (R = Kn B, a per-row finalise); the column side is ONE
 * bigkrls_dev_kernel_contract_grouped (C_g = K(Z[g], X)' B*[g] for all groups), a finalise into S (n x G |J|), and
 * M = S' V S: from the factors T = Q' S (bigkrls_dev_gemm) and M = T' diag(w) T (bigkrls_dev_gram_weighted), from the
 * matrix P = V S and M = S' P. Device memory O(n G (1 + |J|)), never O(u n). */
int bigkrls_group_effects(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                          const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                          const double* h_newdata, int64_t u, const int64_t* h_group, int64_t G,
                          const double* d_vcov_c, const double* d_Q, int64_t ldq, int64_t k, const double* h_w,
                          double* h_derivatives, double* h_ame, double* h_cov);

/* Heteroskedasticity- or cluster-robust variance of the coefficients as factors (no counterpart in the reference).
 * d_Q (n x k, ldq >= n, device) and h_d (k, host) are the kept eigenpairs of the fit, lambda its ridge parameter,
 * h_resid (n, host) the residuals y - yfitted in standardised units, y_sd the standard deviation of y. With
 * g_j = 1 / (d_j + lambda) and G = Q diag(g) Q', the result is V_r = sd(y)^2 scale G diag(omega) G in the units of the
 * fit's vcov.est.c, returned as d_Qout (n x k, ldqo >= n, device; must not overlap d_Q) and h_wout (k, host, descending,
 * >= 0): V_r = Qout diag(wout) Qout'. omega by type, with h_i = sum_j Q_ij^2 d_j g_j the leverages:
 *   0 classical: omega_i = 1 (h_resid unused; scale = sigmasq reproduces the fit's own factors),
 *   1 HC0: e_i^2,   2 HC1: e_i^2 (the caller passes scale = n / Neffective),
 *   3 HC2: e_i^2 / (1 - h_i),   4 HC3: e_i^2 / (1 - h_i)^2; a leverage >= 1 is BIGKRLS_EINVAL naming the row.
 * With h_cluster (n labels in [0, G), host; types 1 and 2 only) the middle is the clustered one,
 * Q' diag(omega) Q -> S S' with S = bigkrls_dev_cluster_scores(Q, e); scale carries the caller's G / (G - 1).
 *   5 CR3 (h_cluster required): the cluster jackknife -- the clustered middle on the deletion residuals
 *     et_S = (I - H_SS)^-1 e_S of every cluster (bigkrls_dev_deletion_residuals) in place of e; the caller passes
 *     scale = (G - 1) / G. A cluster with a block leverage of 1 or more is BIGKRLS_EINVAL naming it.
 * Steps: M = Q' diag(omega) Q (bigkrls_dev_gram_weighted) or S S'; S = diag(g) M diag(g), symmetrised; its k
 * eigenpairs (theta, U) by bigkrls_dev_eigen, theta < 0 (rounding, or rank G < k) set to 0; Qout = Q U, wout =
 * sd(y)^2 scale theta (the scalar stays outside the eigenproblem, so Qout does not depend on it). Workspace beyond the outputs: 3 k^2 + 3 n + k G doubles; bigkrls_dev_gram_weighted's slabs
 * (8 s t 128^2 bytes); with clusters 8 n + 8 pieces bytes of indices and k doubles per piece of a cluster that spans
 * several 64-row chunks, at most k (n / 64 + G) doubles -- n k / 64 above O(k^2 + n + k G); and what bigkrls_dev_eigen
 * and bigkrls_dev_gemm take for a k x k problem and an n x k product.
 * Deterministic: two calls give bitwise identical results. */
int bigkrls_vcov_robust(bigkrls_ctx* ctx, int64_t n, int64_t k, const double* d_Q, int64_t ldq, const double* h_d,
                        double lambda, const double* h_resid, double y_sd, double scale, int32_t type,
                        const int64_t* h_cluster, int64_t G, double* d_Qout, int64_t ldqo, double* h_wout);

/* Case- and cluster-deletion diagnostics of a fitted model (no counterpart in the reference): which observations, or
 * which clusters, the result rests on, without refitting. X, y, coeffs, sigma, h_which, newdata and u as in
 * bigkrls_marginal_effects (validation, standardisation, binary columns and error messages are its own; h_newdata NULL:
 * the training rows); d_Q (n x k, ldq >= n, device) and h_d (k, host) the kept eigenpairs of the fit, lambda its ridge
 * parameter, h_resid (n, host) the residuals in standardised units; h_unit: n labels in [0, G) (host), or NULL: every row
 * is its own unit. U = G, or n. With g = 1 / (d + lambda), w = d g, H = Q diag(w) Q': deleting the rows S of a unit with
 * the basis Q, sigma, lambda and the standardisation HELD AT THEIR FULL-SAMPLE VALUES gives
 *   et_S = (I - H_SS)^-1 e_S,   c - c(-S) = Q diag(g) (Q_S' et_S),   yhat - yhat(-S) = Q diag(w) (Q_S' et_S).
 * Outputs (host; any may be NULL):
 *   h_hat (n): the leverages h_i = sum_m Q_im^2 w_m;
 *   h_resid_deleted, h_fitted_deleted (n): sd(y) et, and y - sd(y) et: every row's prediction by the fit without its unit;
 *   h_cooks (U): sum_m (w_m s_mu)^2 / (tr(H) e'e / (n - tr(H))), s_u = Q_S' et_S, tr(H) = sum w;
 *   h_dfame (U x |J| column-major): AME_j(full) - AME_j(without unit u) in bigkrls_marginal_effects' units, on newdata;
 *   h_ame (|J|): AME_j of the full fit as s_j' c, s_j bigkrls_marginal_effects' column side;
 *   h_var_jack (|J|): ((U - 1) / U) sum_u dfame[u, j]^2, the jackknife variance of the AME -- times the reference's
 *         factor 2 for a binary column (src/bigderiv_v3.cpp:85), as bigkrls_marginal_effects' h_var: with clusters it is
 *         the var.avgderivatives of bigkrls_vcov_robust's type 5;
 *   h_r2_loo (scalar): 1 - sum et^2 / sum ys^2.
 * Steps: bigkrls_dev_deletion_residuals (route 0) with the leverages and, for Cook's distances of clusters, the scores;
 * S by bigkrls_dev_kernel_contract and the marginal effects' finalise, B = Q diag(g) (Q' S) by two bigkrls_dev_gemm,
 * dfame = bigkrls_dev_cluster_scores(B, et)' (single rows: diag(et) B). Device memory O(n (p + |J|) + k U). */
int bigkrls_influence(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y, const double* h_coeffs,
                      double sigma, const int64_t* h_which, int64_t n_which, const double* h_newdata, int64_t u,
                      const double* d_Q, int64_t ldq, int64_t k, const double* h_d, double lambda, const double* h_resid,
                      const int64_t* h_unit, int64_t G, double* h_hat, double* h_resid_deleted, double* h_fitted_deleted,
                      double* h_cooks, double* h_dfame, double* h_ame, double* h_var_jack, double* h_r2_loo);

/* =============================================================================
 * Multi-GPU: one process per GPU, the collectives inside the library (the context's
 * "device list, streams, RCCL comm"; section 8(e): the partitioning). The reference's parallel path is driven from R
 * (PSOCK workers, R/bigKRLS.R:337-363); here the R shim starts one process per GPU, distributes a unique id and
 * every process calls bigkrls_fit_dist with the same X, y and options.
 * ========================================================================== */
typedef struct bigkrls_comm bigkrls_comm;
#define BIGKRLS_UNIQUE_ID_BYTES 128
/* Rank 0: a fresh id (ncclGetUniqueId) for the caller to hand to every rank (sockets, MPI, a file, ...). */
int bigkrls_comm_unique_id(void* id_out_128_bytes);
/* Every rank, concurrently: ncclCommInitRank on the context's device. RCCL (librccl.so) is opened at run time; a
 * missing library gives BIGKRLS_ENODEVICE. nranks == 1 is valid (the collectives then run on one GPU). */
int bigkrls_comm_create(bigkrls_ctx* ctx, int32_t nranks, int32_t rank, const void* unique_id_128_bytes,
                        bigkrls_comm** comm);
/* The same rank object over caller-supplied collectives instead of RCCL: every callback receives DEVICE pointers to
 * doubles (the library has synchronised its stream before the call and expects the result in place at return) and
 * returns 0 on success. op: 0 = sum, 1 = min. Used by the tests to run several ranks on ONE GPU with host-staged
 * collectives; ctx may be NULL for a table that is only passed to bigkrls_comm_check. */
typedef struct bigkrls_collectives {
  int64_t struct_bytes;   /* sizeof(bigkrls_collectives); checked */
  void* user;
  int (*all_reduce)(void* user, double* buf, int64_t count, int32_t op);
  int (*all_gather)(void* user, const double* send, double* recv, int64_t count_per_rank);
  int (*broadcast)(void* user, double* buf, int64_t count, int32_t root);
} bigkrls_collectives;
int bigkrls_comm_create_callbacks(bigkrls_ctx* ctx, int32_t nranks, int32_t rank, const bigkrls_collectives* table,
                                  bigkrls_comm** comm);
int bigkrls_comm_destroy(bigkrls_comm* comm);
/* For hosts whose finalisers run in no particular order (R at exit: r-shim/src/bigkrls_shim.cpp): tell a communicator
 * that its context has ALREADY been destroyed, so that bigkrls_comm_destroy does not synchronise that context's stream. */
int bigkrls_comm_forget_context(bigkrls_comm* comm);
int bigkrls_comm_rank(bigkrls_comm* comm, int32_t* rank, int32_t* nranks);
/* Plumbing check: one all-reduce (sum) of buf[0 .. count), one all-reduce (min) of buf[count .. 2 count), one
 * all-gather of buf[2 count .. 3 count) into buf[4 count .. (4 + nranks) count) and one broadcast from the last rank
 * of buf[3 count .. 4 count); buf is whatever memory the collectives accept (device for RCCL). */
int bigkrls_comm_check(bigkrls_comm* comm, double* buf, int64_t count);
/* The rows [*r0, *r1) this rank owns in a bigkrls_fit_dist call with these sizes and options (blocks of
 * ceil(n / nranks) rows, a multiple of 64 where the dense eigensolver's stage 1 is partitioned): the caller sizes
 * the device outputs with it. */
int bigkrls_fit_dist_rows(bigkrls_comm* comm, int64_t n, const bigkrls_fit_options* options, int64_t* r0, int64_t* r1);
/* bigkrls_fit over the ranks of `comm` (same h_X, h_y, options on every rank): rank r builds and keeps the column
 * block K[:, r0:r1) only -- K is never gathered --, the eigensolver is the block Lanczos with sharded K B_j products
 * (Neig << N) or the dense path with stage 1 partitioned by column blocks, lambda search / coefficients / fitted
 * values / variance matrices / marginal effects work on the row block with one all-reduce or all-gather each.
 * Every rank receives the same small host outputs; the device outputs d_K, d_vcov_c, d_vcov_fitted are this rank's
 * COLUMN blocks (n x (r1 - r0), ld n); d_vcov_q / vcov_w (the factors of vcov.est.c) are whole on every rank.
 * BIGKRLS_DIST_EIGEN=krylov|dense|replicated overrides the choice of the eigensolver (development / tests). */
int bigkrls_fit_dist(bigkrls_comm* comm, const double* h_X, const double* h_y, int64_t n, int64_t p,
                     const bigkrls_fit_options* options, bigkrls_fit_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* BIGKRLS_H */
