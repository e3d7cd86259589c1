/*
 * viprs_hip.h -- C ABI of libviprs_hip.so: the MI355X (gfx950) implementation of viprs's
 * coordinate-ascent variational E-step over LD-matrix blocks.
 *
 * This header is the drop-in boundary.  Every entry point names the reference interface it
 * replaces (paths relative to the shz9/viprs tree, v0.1.4):
 *
 *   reference (Cython -> C++ templates)                         this library
 *   ----------------------------------------------------------  -------------------------------
 *   e_step_cpp.pyx:91-122   cpp_e_step          -> e_step.hpp:343-442   viprs_e_step
 *   e_step_cpp.pyx:125-159  cpp_e_step_mixture  -> e_step.hpp:447-551   viprs_e_step_mixture
 *   e_step_cpp.pyx:161-195  cpp_e_step_grid     -> e_step.hpp:555-647   viprs_e_step_grid
 *   e_step_cpp.pyx:71-76    check_blas_support / check_omp_support      viprs_check_*_support
 *   VIPRS.py:151-172        "load LD matrices to memory" (VIPRS.__init__) viprs_plan_create
 *   VIPRS.py:393-422        per-chromosome loop in VIPRS.e_step()       viprs_state_* (resident)
 *
 * Conventions
 *   - plain pointers + sizes + dtype codes; no C++/torch types cross this boundary;
 *   - every function returns 0 on success, a negative VIPRS_E* code otherwise;
 *     viprs_last_error() returns a thread-local message for the last failure;
 *   - host buffers stay caller-owned; device mirrors are owned by the opaque handles;
 *   - results always follow the reference's `threads = 1` (exact serial Gauss-Seidel)
 *     semantics; the `threads` argument is accepted for signature parity and ignored
 *     (the reference's threads > 1 path is a racy Hogwild loop, e_step.hpp:384-387).
 */
#ifndef VIPRS_HIP_H
#define VIPRS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dtype codes (mirror the Cython fused types, e_step_cpp.pxd:7-17) ------------------- */
enum viprs_float_dtype { VIPRS_F32 = 0, VIPRS_F64 = 1 };               /* `floating`          */
enum viprs_ld_dtype {                                                   /* noncomplex_numeric  */
    VIPRS_LD_I8 = 0, VIPRS_LD_I16 = 1, VIPRS_LD_I32 = 2, VIPRS_LD_I64 = 3,
    VIPRS_LD_F32 = 4, VIPRS_LD_F64 = 5
};
enum viprs_indptr_dtype { VIPRS_IP_I32 = 0, VIPRS_IP_I64 = 1 };        /* indptr_type         */

/* ---- status codes ----------------------------------------------------------------------- */
enum viprs_status {
    VIPRS_OK = 0,
    VIPRS_EINVAL = -1,     /* bad argument / dtype code                                        */
    VIPRS_ELAYOUT = -2,    /* LD index arrays violate the contiguous-window contract            */
    VIPRS_EDEVICE = -3,    /* HIP runtime error (message in viprs_last_error)                   */
    VIPRS_ENOMEM = -4,
    VIPRS_EUNSUPPORTED = -5
};

/* ---- E-step numerics mode ---------------------------------------------------------------- */
enum viprs_math_mode {
    /* Bit-for-bit the reference's arithmetic (glibc-2.35 expf reproduced in double on the
     * device, sigmoid divide in double as e_step.hpp:254-260 does).  Default.                 */
    VIPRS_MATH_EXACT = 0,
    /* Hardware v_exp_f32 / v_rcp_f32 sigmoid (<= 2 ulp from EXACT per evaluation; well inside
     * the 1e-5 relative parity tolerance).  Shorter serial chain per SNP.                     */
    VIPRS_MATH_FAST = 1
};

/* ---- block kinds reported by the planner ------------------------------------------------- */
enum viprs_block_kind {
    VIPRS_BLOCK_DENSE_SYM = 0,    /* every row's window == the whole block (symmetric form)    */
    VIPRS_BLOCK_DENSE_UPPER = 1,  /* row j's window == (j, block_end)      (upper-tri form)    */
    VIPRS_BLOCK_RAGGED = 2        /* anything else (banded / thresholded windows)              */
};

typedef struct viprs_plan viprs_plan;     /* device-resident LD + block schedule               */
typedef struct viprs_state viprs_state;   /* device-resident variational state bound to a plan */

/* ---- library / device ------------------------------------------------------------------- */
const char* viprs_last_error(void);
const char* viprs_version(void);
/* Experiment / instrumentation switches (-DPANEL_TIMING_*, -DVIPRS_*_PROFILE, ...: kernels_common.h) the translation
 * units of this library were compiled with, space separated.  The shipped library returns "": some of those switches
 * change results, a build that carries any is not the product (they do not compile without -DVIPRS_EXPERIMENTAL). */
const char* viprs_build_flags(void);
int viprs_device_count(int* count);
/* Mirrors check_blas_support() / check_omp_support() (e_step_cpp.pyx:71-76): neither BLAS
 * nor OpenMP is involved on the device path, both report 0.                                   */
int viprs_check_blas_support(void);
int viprs_check_omp_support(void);

/* Content fingerprint of a HOST array: length + first / last 4 KB + 256 evenly spaced 64-byte windows (pure host code, a few
 * microseconds).  The Cython entry points read the caller's LD arrays on every call (e_step_cpp.pyx:91-122); a binding that
 * keeps them resident on the device uses this to notice an in-place edit (viprs_amd/vi/e_step_hip.py::plan_for).            */
int viprs_host_fingerprint(const void* data, int64_t n_bytes, uint64_t* fingerprint);

/* ---- planner (pure host code; usable without a GPU) -------------------------------------- */
/* Validates the LD index arrays (bit-exact integer checks: indptr[0] == 0, indptr monotone,
 * 0 <= left_bound[j], left_bound[j] + len_j <= m; symmetric form: window contains j;
 * upper form: left_bound[j] == j + 1) and partitions SNPs 0..m-1 into independent LD blocks
 * (= connected components of the row windows; the reference has no explicit block loop,
 * independence is implicit in (left_bound, indptr): e_step.hpp:389-392).
 *
 *   block_start  out, capacity m + 1: block b covers SNPs [block_start[b], block_start[b+1])
 *   block_kind   out, capacity m (may be NULL)
 */
int viprs_plan_blocks(int64_t m, const int32_t* ld_left_bound, const void* ld_indptr,
                      int indptr_dtype, int low_memory, int64_t* n_blocks, int64_t* block_start,
                      int32_t* block_kind);

/* ---- plan: upload LD once (replaces "load LD to memory", VIPRS.py:151-172) ---------------- */
int viprs_plan_create(viprs_plan** plan, int64_t m, const int32_t* ld_left_bound,
                      const void* ld_indptr, int indptr_dtype, const void* ld_data, int ld_dtype,
                      int low_memory, int device);
/* Symmetric plan (the `low_memory = False` arithmetic, e_step.hpp:421-428) built from the compact
 * UPPER-TRIANGULAR store: row j of `upper_data` holds the correlations with SNPs j+1 .. j+len_j
 * (`upper_indptr`, m + 1 entries), as LD matrices are kept on disk.  The store is uploaded once and
 * mirrored into the symmetric windows on the device; `diag_value` fills the diagonal (1 for float
 * LD, the quantisation maximum -- 127 / 32767 -- for integer LD).  Replaces the host-side
 * `ld_mat.load(return_symmetric=True)` of VIPRS.py:167-172: the symmetric copy never exists in host
 * memory and half the bytes cross PCIe.  The right ends j + len_j must not decrease (otherwise the
 * mirrored rows would not be contiguous windows): VIPRS_EINVAL.
 * viprs_plan_get_windows returns the (left_bound, indptr) arrays of the plan's rows (any plan). */
int viprs_plan_create_expanded(viprs_plan** plan, int64_t m, const void* upper_indptr, int indptr_dtype,
                               const void* upper_data, int ld_dtype, double diag_value, int device);
int viprs_plan_get_windows(const viprs_plan* plan, int32_t* left_bound, int64_t* indptr);
int viprs_plan_destroy(viprs_plan* plan);

enum viprs_plan_info_key {
    VIPRS_INFO_M = 0, VIPRS_INFO_NNZ = 1, VIPRS_INFO_N_BLOCKS = 2, VIPRS_INFO_N_DENSE = 3,
    VIPRS_INFO_N_RAGGED = 4, VIPRS_INFO_MAX_BLOCK = 5, VIPRS_INFO_LD_BYTES_DEVICE = 6,
    VIPRS_INFO_LD_ELEM_SIZE = 7, VIPRS_INFO_DEVICE = 8, VIPRS_INFO_LOW_MEMORY = 9,
    VIPRS_INFO_N_CU = 10,
    /* upper form: 1 while the dense blocks hold the upper triangle mirrored into the lower one (the fp32 sweeps' storage),
     * 0 while the lower triangle is zero (as created; the float64 sweeps' storage) */
    VIPRS_INFO_UPPER_MIRRORED = 11
};
int viprs_plan_info(const viprs_plan* plan, int key, int64_t* value);
/* Copies the planner's block boundaries (n_blocks + 1 entries) */
int viprs_plan_get_blocks(const viprs_plan* plan, int64_t* block_start, int32_t* block_kind);
int viprs_plan_set_math_mode(viprs_plan* plan, int math_mode);
/* Which LD blocks the following sweeps visit: one byte per block in SNP order (the order of viprs_plan_get_blocks), non-zero =
 * swept; NULL = every block again.  The reference fits one model per chromosome by default (bin/viprs_fit:232-238, fan-out
 * :1079-1086) and each of those fits stops at its own iteration (VIPRS.py:1046-1094); with the chromosomes' blocks in ONE
 * plan (viprs_state_set_groups below) a converged chromosome's blocks leave the sweep this way -- its state stays as its
 * last E-step left it.  Host-side list surgery over a few thousand descriptors; LD and per-SNP arrays do not move.
 * Every kernel family sweeps the active subset, the batched grid kernel included (it rebuilds its teams from the new list). */
int viprs_plan_set_active_blocks(viprs_plan* plan, const uint8_t* active, int64_t n_blocks);

/* ---- one-shot calls on host buffers: the drop-ins for the Cython entry points ------------ */
/* Argument order and meaning follow e_step_cpp.pyx:91-122 after the plan handle (which stands
 * for ld_left_bound / ld_indptr / ld_data).  var_gamma, var_mu, eta, q, eta_diff are updated
 * in place exactly as e_step.hpp:343-442 does; all float buffers share `float_dtype`.         */
int viprs_e_step(viprs_plan* plan, int float_dtype, const void* std_beta, void* var_gamma,
                 void* var_mu, void* eta, void* q, void* eta_diff, const void* u_logs,
                 const void* sqrt_half_var_tau, const void* mu_mult, double dq_scale, int threads,
                 int low_memory);

/* e_step_cpp.pyx:125-159: (m, K) arrays are C-ordered.                                        */
int viprs_e_step_mixture(viprs_plan* plan, int float_dtype, int K, const void* std_beta,
                         void* var_gamma, void* var_mu, void* eta, void* q, void* eta_diff,
                         const void* log_null_pi, const void* u_logs,
                         const void* sqrt_half_var_tau, const void* mu_mult, double dq_scale,
                         int threads, int low_memory);

/* e_step_cpp.pyx:161-195: (m, G) arrays are column-major; active_model_idx is contiguous here
 * (the ctypes shim gathers a strided int[:]).                                                 */
int viprs_e_step_grid(viprs_plan* plan, int float_dtype, int G, const void* std_beta,
                      void* var_gamma, void* var_mu, void* eta, void* q, void* eta_diff,
                      const void* u_logs, const void* half_var_tau, const void* mu_mult,
                      double dq_scale, const int32_t* active_model_idx, int n_active, int threads,
                      int low_memory);

/* ---- device-resident state: what VIPRS.e_step()'s per-iteration loop keeps alive --------- */
enum viprs_model_kind { VIPRS_MODEL_SPIKE_SLAB = 0, VIPRS_MODEL_MIXTURE = 1, VIPRS_MODEL_GRID = 2 };

enum viprs_field {
    /* inputs */
    VIPRS_FIELD_STD_BETA = 0, VIPRS_FIELD_U_LOGS = 1, VIPRS_FIELD_SQRT_HALF_VAR_TAU = 2,
    VIPRS_FIELD_MU_MULT = 3, VIPRS_FIELD_LOG_NULL_PI = 4,
    /* in/out state */
    VIPRS_FIELD_VAR_GAMMA = 5, VIPRS_FIELD_VAR_MU = 6, VIPRS_FIELD_ETA = 7, VIPRS_FIELD_Q = 8,
    VIPRS_FIELD_ETA_DIFF = 9,
    VIPRS_FIELD_COUNT = 10,
    /* the two inputs of the elastic-net sweep (viprs_state_enet_sweep) live in fields of the E-step */
    VIPRS_FIELD_ENET_MULT = VIPRS_FIELD_MU_MULT,                  /* c_j: lassosum's 1 - s */
    VIPRS_FIELD_ENET_PENALTY = VIPRS_FIELD_SQRT_HALF_VAR_TAU      /* pen_j >= 0: lambda times an optional per-SNP factor */
};

/* `width` = 1 (spike-and-slab), K (mixture) or G (grid).                                      */
int viprs_state_create(viprs_state** state, viprs_plan* plan, int float_dtype, int model_kind,
                       int width);
int viprs_state_destroy(viprs_state* state);
/* Whole-field copies; sizes follow the reference shapes ((m,), (m,K) C-order, (m,G) F-order).  */
int viprs_state_upload(viprs_state* state, int field, const void* host);
int viprs_state_download(viprs_state* state, int field, void* host);
/* Device-side re-initialisation to the reference's standard start (VIPRS.py:344-358):
 * var_gamma = pi, var_mu = eta = q = eta_diff = 0.                                            */
int viprs_state_reset(viprs_state* state, double pi);
/* One E-step sweep over every LD block with the resident inputs; asynchronous on the plan's
 * stream unless `sync` != 0.                                                                  */
int viprs_state_e_step(viprs_state* state, double dq_scale, const int32_t* active_model_idx,
                       int n_active, int sync);
int viprs_state_synchronize(viprs_state* state);

/* ---- device-resident EM iteration (spike-and-slab): host prep, zeta and the M-step / ELBO sums ---
 * Replaces the O(m) NumPy passes of VIPRS.e_step / compute_zeta / m_step / elbo
 * (VIPRS.py:400-418, :888-897, :426-471, :497-581) so that fit() moves only scalars per iteration. */
/* n_per_snp (float64, (m,)), uploaded once.                                                      */
int viprs_state_set_n_per_snp(viprs_state* state, const double* n_per_snp);
/* On-device VIPRS.py:400-418 in float64, rounded to the state precision at the end:
 *   var_tau = n one_plus_lambda / sigma_epsilon + tau_beta
 *   mu_mult = n / (var_tau sigma_epsilon);  sqrt_half_var_tau = sqrt(var_tau / 2)
 *   u_logs  = logit_pi + 0.5 (log_tau_beta - log var_tau)
 * (the scalars logit_pi = log(pi) - log(1 - pi), log_tau_beta and one_plus_lambda = 1 + lambda_min
 * are evaluated by the caller so that the reference's scalar dtype promotion -- float32 scalars in
 * VIPRS.py:400-406 -- can be reproduced exactly).                                                 */
int viprs_state_prep(viprs_state* state, double logit_pi, double log_tau_beta, double sigma_epsilon,
                     double tau_beta, double one_plus_lambda);
/* Deterministic (fixed-order) float64 reductions over the plan's SNPs with the hyper-parameters of
 * the last viprs_state_prep; `out` receives VIPRS_N_SUMS doubles on the HOST:
 *   [0] sum gamma  [1] sum zeta  [2] sum(one_plus_lambda zeta + q eta)  [3] sum std_beta eta  [4] sum eta^2
 *   [5] sum g log g  [6] sum (1-g) log(1-g)  [7] sum g  [8] sum (1-g)   (g clipped to [1e-15, 1-1e-15])
 *   [9] sum g log var_tau  [10] max |eta_diff|
 * zeta = gamma (mu^2 + 1/var_tau) in float64 (VIPRS.py:896).  Synchronises the plan's stream.
 * THE ORDER, for every sums call of this header (a "row" is what one output row is summed over: the plan, a grid
 * column, an SNP group, a (group, column) pair): a row of `len` SNPs takes nb = min(ceil(len / 256), cap) workgroups of
 * 256 threads, cap = 1024 (spike-and-slab and mixture rows) or 256 (rows of a grid state).  Thread t of workgroup b adds
 * the terms of SNPs b * 256 + t, + nb * 256, + 2 nb * 256, ... serially (ceil(len / (nb * 256)) additions); the workgroup
 * combines its 256 accumulators in a binary tree (8 levels; mixture rows: 6 levels within each wave, then the 4 waves in
 * order); a final pass adds the nb partials, lane l of 64 taking partials l, l + 64, ... serially (ceil(nb / 64)
 * additions), then a 6-level tree over the lanes.  So the longest path of a row has
 *   D = ceil(len / (nb * 256)) + 8 (mixture: 9) + ceil(nb / 64) + 6
 * additions, every sum is within 2^-52 (D + C) sum |terms| of the exact sum of its terms (C: the rounded operations in
 * one term), and it depends on nothing but the row's own SNPs: not on the other rows of the call, their number or
 * order, nor on timing.  A row of no SNPs (an empty group) returns zeros.  The maximum [10] ignores NaNs (fmax).        */
#define VIPRS_N_SUMS 11
/* Optional per-SNP weights (m doubles; NULL clears them) for sum [0]: with several chromosomes merged into one
 * plan, w_j = 1 / (SNPs of j's chromosome) makes sum [0] the reference's sum of per-chromosome means
 * (update_pi, VIPRS.py:446-453). */
int viprs_state_set_snp_weights(viprs_state* state, const double* weights);
int viprs_state_sums(viprs_state* state, double one_plus_lambda, double* out);
/* The same in two halves, so that several plans (chromosomes) reduce concurrently: `begin` enqueues the
 * reduction and an asynchronous copy on the plan's stream, `end` waits for it and returns the sums. */
int viprs_state_sums_begin(viprs_state* state, double one_plus_lambda);
int viprs_state_sums_end(viprs_state* state, double* out);
/* The same two operations on ONE model (column `g`) of a grid state ((m, G) column-major arrays),
 * for the batched grid fit: e_step_grid takes half_var_tau = var_tau / 2 (e_step.hpp:616) where
 * e_step takes its square root, otherwise the formulas are those above.  (A grid state does not keep
 * var_tau -- m x G doubles written per prep and read back per reduction: the sums form it again from n_j
 * and the scalars of the column's last prep, the same expression, the same bits.)                   */
int viprs_state_prep_column(viprs_state* state, int g, double logit_pi, double log_tau_beta, double sigma_epsilon,
                            double tau_beta, double one_plus_lambda);
int viprs_state_sums_column(viprs_state* state, int g, double one_plus_lambda, double* out);
/* ---- device-resident EM iteration of the mixture model (K <= 8), VIPRSMix.py:169-260 -------------------
 * prep    : var_tau[j,k] = n_j * one_plus_lambda / sigma_epsilon + tau_beta[k] and the E-step inputs of the state
 *           (u_logs, sqrt_half_var_tau, mu_mult, log_null_pi).  The K-vectors logit_pi = log(pi) - log(1 - pi),
 *           log_tau_beta and tau_beta and the scalar log_null_pi are evaluated by the caller (reference dtype
 *           semantics).  Needs viprs_state_set_n_per_snp.
 * log_var_tau : (m, K) doubles, C order -- log of the INITIAL var_tau, which the reference's ELBO keeps using.
 * sums    : 7 + 6 K doubles: sum zeta | sum((1+lambda) zeta + q eta) | sum std_beta eta | sum eta^2 |
 *           sum null_gamma log null_gamma | sum null_gamma | then K-vectors sum gamma | sum gamma (mu^2 + 1/var_tau) |
 *           sum gamma_c log gamma_c | sum gamma_c | sum gamma_c log_var_tau | sum gamma_c (mu^2 + 1/var_tau)
 *           (gamma_c = gamma clipped to [1e-15, 1 - 1e-15]) | max |eta_diff|. */
int viprs_state_set_log_var_tau(viprs_state* state, const double* log_var_tau);
int viprs_state_prep_mixture(viprs_state* state, const double* logit_pi, const double* log_tau_beta,
                             const double* tau_beta, double log_null_pi, double sigma_epsilon, double one_plus_lambda);
int viprs_state_sums_mixture_begin(viprs_state* state, double one_plus_lambda);
int viprs_state_sums_mixture_end(viprs_state* state, double* out);

/* Several models per launch (the batched grid fit touches every active model in every EM iteration):
 *   params : n rows of 6 doubles  (column, logit_pi, log_tau_beta, sigma_epsilon, tau_beta, one_plus_lambda)
 *   cols   : n rows of 2 doubles  (column, one_plus_lambda)
 *   out    : n rows of VIPRS_N_SUMS doubles, in the order of `cols`
 * `begin` is asynchronous on the plan's stream, `end` waits for it. */
int viprs_state_prep_columns(viprs_state* state, int n, const double* params);
int viprs_state_sums_columns_begin(viprs_state* state, int n, const double* cols);
int viprs_state_sums_columns_end(viprs_state* state, double* out);
/* Per-column re-initialisation of a grid state: var_gamma[:, g] = pi_g, everything else 0.         */
int viprs_state_reset_column(viprs_state* state, int g, double pi);

/* ---- SNP groups: one spike-and-slab model per chromosome, all chromosomes in ONE plan -----------------------------
 * The reference's default mode (bin/viprs_fit:232-238: `split_by_chromosome()` unless --genomewide) fits an independent
 * VIPRS model per chromosome, each with its own (pi, tau_beta, sigma_epsilon), M-step sums, ELBO and stopping iteration.
 * A chromosome-sized fit cannot fill the device (its sweep is bound by the chain of its largest LD block), 22 of them in
 * one plan cost one genome-wide sweep.  A GROUP is a contiguous SNP range made of whole LD blocks:
 *   viprs_state_set_groups        group g = SNPs [group_start[g], group_start[g+1]); n_groups + 1 entries covering 0 .. m;
 *                                 n_groups = 0 removes the groups.  Spike-and-slab, mixture (K <= 8) and grid states.
 *   viprs_state_prep_groups       viprs_state_prep with per-group scalars: n rows of 6 doubles
 *                                 (group, logit_pi, log_tau_beta, sigma_epsilon, tau_beta, one_plus_lambda); only the listed
 *                                 groups' SNPs are rewritten (a converged group keeps the inputs of its last E-step).
 *   viprs_state_sums_groups_begin n rows of 2 doubles (group, one_plus_lambda): the VIPRS_N_SUMS sums of viprs_state_sums
 *                                 per listed group, one launch; [0] is the plain sum of gamma (no per-SNP weights).
 *   viprs_state_sums_groups_end   n rows of VIPRS_N_SUMS doubles in the order of the rows given to `begin`.
 * A group's inputs and sums are bit-identical to those of a plan that holds only that group's blocks (the reduction over
 * a group uses the workgroup count and element order a plan of that size would use).  With viprs_state_set_comm the rows
 * are all-rank sums (one all-gather for all groups). */
int viprs_state_set_groups(viprs_state* state, int n_groups, const int64_t* group_start);
int viprs_state_prep_groups(viprs_state* state, int n, const double* params);
int viprs_state_sums_groups_begin(viprs_state* state, int n, const double* rows);
int viprs_state_sums_groups_end(viprs_state* state, double* out);
/* The same for a mixture state (one VIPRSMix model per chromosome; K = the state's width):
 *   viprs_state_prep_mixture_groups       viprs_state_prep_mixture with per-group parameters: n rows of 4 + 3 K doubles
 *                                         (group, log_null_pi, sigma_epsilon, one_plus_lambda, logit_pi[K], log_tau_beta[K],
 *                                         tau_beta[K])
 *   viprs_state_sums_mixture_groups_begin n rows of 2 doubles (group, one_plus_lambda)
 *   viprs_state_sums_mixture_groups_end   n rows of 7 + 6 K doubles, the layout of viprs_state_sums_mixture_end
 * viprs_state_set_log_var_tau takes the (m, K) array of all groups as before. */
int viprs_state_prep_mixture_groups(viprs_state* state, int n, const double* params);
int viprs_state_sums_mixture_groups_begin(viprs_state* state, int n, const double* rows);
int viprs_state_sums_mixture_groups_end(viprs_state* state, double* out);
/* The same for a GRID state (one VIPRSGrid per chromosome, every grid point fitted from the standard start): one set of
 * hyper-parameters per (group, column) pair -- a group is a chromosome, a column a grid point.
 *   viprs_state_prep_grid_groups          viprs_state_prep_columns per pair: n rows of 7 doubles (group, column, logit_pi,
 *                                         log_tau_beta, sigma_epsilon, tau_beta, one_plus_lambda); only the listed pairs'
 *                                         SNPs x column are rewritten; each pair's scalars are kept for its sums (a grid
 *                                         state keeps no var_tau, see viprs_state_prep_column)
 *   viprs_state_sums_grid_groups_begin    n rows of 3 doubles (group, column, one_plus_lambda): the VIPRS_N_SUMS sums per pair
 *                                         in one launch, [0] the plain sum of gamma
 *   viprs_state_sums_grid_groups_end      n rows of VIPRS_N_SUMS doubles in the order of the rows given to `begin`
 *   viprs_state_set_group_columns         n_groups x width row-major mask (non-zero = on); n_groups = 0 clears it.  Under a
 *                                         mask, viprs_state_e_step sweeps column g of group c only if g is in
 *                                         active_model_idx AND active[c][g] is set; every other pair keeps every bit of its
 *                                         var_gamma / var_mu / eta / q / eta_diff.  fp32 states on dense blocks (the batched
 *                                         matrix-core kernel and the panel kernel); float64 states and ragged / banded blocks
 *                                         under a mask: VIPRS_EUNSUPPORTED.
 * A pair's inputs, sweep and sums are bit-identical to those of column `column` of a grid state whose plan holds only that
 * group's blocks (swept with that group's active list).  viprs_state_set_groups clears the pairs' scalars and the mask. */
int viprs_state_prep_grid_groups(viprs_state* state, int n, const double* params);
int viprs_state_sums_grid_groups_begin(viprs_state* state, int n, const double* rows);
int viprs_state_sums_grid_groups_end(viprs_state* state, double* out);
int viprs_state_set_group_columns(viprs_state* state, int n_groups, int width, const uint8_t* active);

/* ---- committing SNP groups into grid columns: the pathwise grid search per chromosome ----------------------------------
 * A chromosome (an SNP group of a spike-and-slab state) whose grid point has stopped stores its state as one column of a grid
 * state that serves as the result store (never swept; it takes the source's group table).
 *   viprs_state_commit_groups   `pairs`: n rows of 2 int32 (group, column).  For each row, SNPs [group_start[group],
 *                               group_start[group+1]) of var_gamma / var_mu / eta / q / eta_diff of `src` are copied into
 *                               column `column` of the same fields of `dst` (column-major: one contiguous range per field).
 *                               `src`: a spike-and-slab state with groups set (viprs_state_set_groups); `dst`: a grid state on
 *                               the same plan with the same float dtype.  ONE kernel launch for every row and field, on the
 *                               plan's stream behind the work already enqueued (the sweep and sums that produced the state):
 *                               no stream synchronisation, nothing passes through host memory.  The rows travel through the
 *                               source's pinned staging of batched prep rows.  Null handles, different plans, different
 *                               dtypes, wrong model kinds, groups not set, a group or column out of range and n < 0:
 *                               VIPRS_EINVAL before any launch, `dst` untouched. */
int viprs_state_commit_groups(viprs_state* dst, const viprs_state* src, int n, const int32_t* pairs);

/* ---- multi-GPU: RCCL over xGMI for the scalar reductions of the EM iteration -------------------------
 * One process per GPU; LD blocks are sharded over the ranks (independent units: within one E-step call
 * the hyper-parameters are fixed and blocks share no q entries, so the data path has NO collective).
 * What the ranks must agree on per EM iteration are the ~10-300 float64 partial sums of the M-step, the
 * ELBO and the stopping rules (VIPRS.py:426-484, :497-581, :997) -- the reference itself has no collective
 * at all (one process, OpenMP inside the kernel, joblib over chromosomes: bin/viprs_fit:1080-1086).
 *
 * The communicator wraps an RCCL (ncclComm_t) communicator; librccl is opened at run time, so processes
 * that never create a communicator do not load it.  Every reduction is ONE ncclAllGather of the small
 * vector followed by a rank-ordered reduction on the device: sums are added in rank order 0..n-1 (so every
 * rank gets bit-identical results, run to run), the last element of every `group` consecutive elements is
 * reduced with max (that slot carries max |eta_diff|).
 *
 *   viprs_comm_unique_id   rank 0: fills `id` (VIPRS_COMM_ID_BYTES) -- hand it to the other ranks out of band
 *                          (viprs_amd.parallel does it through the file system / the launcher's environment)
 *   viprs_comm_create      collective over all `world_size` processes; `device` = this rank's HIP device
 *   viprs_comm_allreduce   host vector in/out (control plane: hyper-parameter broadcast, bench timing);
 *                          group = 0: plain sum, group = -1: plain max, group > 0: see above
 *   viprs_comm_barrier     all ranks' devices idle + all ranks arrived
 *   viprs_state_set_comm   from now on viprs_state_sums*_begin/_end of this state return the ALL-RANK sums:
 *                          the all-gather + ordered reduction run on the plan's stream between the local
 *                          reduction kernels and the copy to the host -- one collective per EM iteration,
 *                          no host round trip in front of it.  NULL detaches.  A rank whose plan is empty
 *                          still takes part (it contributes zeros).                                          */
#define VIPRS_COMM_ID_BYTES 128
typedef struct viprs_comm viprs_comm;
int viprs_comm_unique_id(void* id);
int viprs_comm_create(viprs_comm** comm, const void* id, int rank, int world_size, int device);
int viprs_comm_destroy(viprs_comm* comm);
int viprs_comm_rank(const viprs_comm* comm, int* rank, int* world_size);
int viprs_comm_allreduce(viprs_comm* comm, double* vec, int n, int group);
/* bulk exchange at the END of a fit (the posterior of each rank's SNPs, BayesPRSModel.py:333-410 wants all of them):
 * every rank sends `n` doubles, `recv` receives world_size x n in rank order -- one ncclAllGather.                    */
int viprs_comm_allgather(viprs_comm* comm, const double* send, int64_t n, double* recv);
int viprs_comm_barrier(viprs_comm* comm);
int viprs_state_set_comm(viprs_state* state, viprs_comm* comm);
/* hipDeviceSynchronize() on `device` (what the bench brackets its timed region with).                   */
int viprs_device_synchronize(int device);

/* ---- measurement hooks (bench.py) --------------------------------------------------------- */
/* HIP-event time (ms) of the kernels of the last viprs_state_e_step / viprs_e_step* call on
 * this plan, measured on the stream they were launched on.  `which`: 0 = all kernels of the
 * sweep, 1 = dominant (panel) kernel only, 2 = HOST time the library spent between recording that
 * kernel's start event and recording its end event (the launch call: a start event recorded into
 * an empty stream is reached at once, so host time spent there counts into the event bracket).
 * A sweep that brackets no dominant kernel -- a spike-and-slab sweep over windowed blocks only -- reports
 * 0 for `which` = 1 and 2, whatever the sweeps before it did.                                   */
int viprs_plan_last_kernel_ms(viprs_plan* plan, int which, double* ms);
/* Every sweep records its HIP events into a ring of 256 entries.  `timing_reset` forgets them;
 * `timing_history` returns the durations (ms) of the most recent min(capacity, 256, recorded)
 * sweeps, oldest first.                                                                       */
int viprs_plan_timing_reset(viprs_plan* plan);
int viprs_plan_timing_history(viprs_plan* plan, int which, double* ms, int capacity, int* n);
/* Arithmetic the kernels of the last sweep on this plan really ran in: bit 0 = exact, bit 1 = fast.
 * viprs_plan_set_math_mode(FAST) applies where a fast instantiation exists (spike-and-slab, grid, mixtures of up to 8
 * components, fp32 state); mixtures of 9+ components, the mixture / grid kernels of windowed blocks with K > 8 and
 * every float64 state run exact whatever was asked for -- this is how a caller (bench.py) finds out.          */
int viprs_plan_last_math_modes(const viprs_plan* plan, int* mask);
/* Number of SNPs of the last sweep that took the skip branch (e_step.hpp:410-413).            */
int viprs_plan_last_skipped(viprs_plan* plan, int64_t* n_skipped);
/* The route of a sweep (pure host code; usable without a GPU): which kernel family a configuration takes and which HIP
 * events the sweep records.  In: the state's precision, model kind and width (K or G), the LD element type, whether the
 * plan's active dense / windowed block lists are non-empty, and three switches -- `band_ok`: VIPRS_BAND is not 0, the LD
 * type is fp32 / int8 / int16 and the widest window fits the band kernel's q ring; `grid_mfma`: the batched grid kernel is
 * on (VIPRS_GRID_MFMA, or by default enough dense blocks to fill the chip); `f64_row_by_row`: VIPRS_F64_ROW_BY_ROW is set.
 * Out: `route[VIPRS_ROUTE_COUNT]`.  VIPRS_EINVAL with the launcher's message when the family the configuration leads to
 * has no instantiation for the LD element type.                                                                       */
enum viprs_sweep_family {
    VIPRS_FAMILY_NONE = 0,           /* no launcher is called for the list */
    VIPRS_FAMILY_GENERIC = 1,        /* row-by-row kernels (called for an empty list too: they return at once) */
    VIPRS_FAMILY_TILE_F64 = 2,       /* float64 states: the panel-walking kernels (likewise) */
    VIPRS_FAMILY_PANEL = 3,          /* the panel sweep; model 0 spike-and-slab, 1 grid column, 2 mixture K <= 8, 3 mixture K <= 31
                                        (4: the elastic net, viprs_enet_route only; 5: the Gibbs draw, viprs_gibbs_route only; 6: SBayesR,
                                        viprs_bayesr_route only) */
    VIPRS_FAMILY_BAND = 4,           /* band kernel of the windowed blocks; model 0 spike-and-slab, 1 grid column, 2 mixture
                                        (3: the elastic net, viprs_enet_route only; 4: the Gibbs draw, viprs_gibbs_route only; 5: SBayesR,
                                        viprs_bayesr_route only) */
    VIPRS_FAMILY_GRID_BATCHED = 5    /* batched grid kernel on the matrix cores: one launch per 32 active columns, a 1-model
                                        prologue launch in front of every launch after the first */
};
enum viprs_route_field {
    VIPRS_ROUTE_DENSE_FAMILY = 0, VIPRS_ROUTE_DENSE_MODEL = 1,      /* the generic and tile families take the model kind */
    VIPRS_ROUTE_RAGGED_FAMILY = 2, VIPRS_ROUTE_RAGGED_MODEL = 3,
    VIPRS_ROUTE_PROLOGUE = 4,                 /* the launch that zeroes queue heads, skip count and hand-off granules */
    VIPRS_ROUTE_PROLOGUE_PER_MODEL = 5,       /* ... granules for every active model (grid), not for one */
    VIPRS_ROUTE_START_EVENT_BY_LAUNCHER = 6,  /* the dominant kernel's start event is recorded adjacent to its launch */
    VIPRS_ROUTE_WHOLE_SWEEP_EVENTS = 7,       /* an event pair around everything beside the dominant kernel's own pair;
                                                 0: that pair goes around all kernels of the call and stands for both */
    VIPRS_ROUTE_DENSE_BRACKETED = 8,          /* the dominant kernel's pair is recorded at all */
    VIPRS_ROUTE_COUNT = 9
};
int viprs_sweep_route(int float_dtype, int model_kind, int width, int ld_dtype, int dense, int ragged, int band_ok,
                      int grid_mfma, int f64_row_by_row, int* route);

/* ---- elastic net (lassosum): cyclic coordinate descent on the sweep of the E-step ------------------------------------------
 * lassosum (Mak et al. 2017) estimates effects from marginal effects and an LD panel by minimising
 *   beta' ((1 - s) R + s I) beta - 2 beta' std_beta + 2 sum_j pen_j |beta_j|
 * by cyclic coordinate descent over each LD block with a running q = (R - I) beta: the serial Gauss-Seidel chain of
 * viprs_state_e_step with a soft threshold where the E-step has a sigmoid.  The reference has no such model; the definition
 * is this library's own, stated in full.
 *   viprs_state_enet_sweep  one sweep over every LD block the plan's sweeps visit (viprs_plan_set_active_blocks filters it
 *                           as it filters the E-step), on an fp32 state of kind VIPRS_MODEL_SPIKE_SLAB (width 1) or
 *                           VIPRS_MODEL_GRID (width G: every column its own c, pen, eta, q); asynchronous on the plan's
 *                           stream unless `sync` != 0
 * THE UPDATE.  Per SNP j in index order, and per column of a grid state, from the current q_j, every operation separately
 * rounded in float32, no fused multiply-add:
 *   t = fl(c_j * q_j)
 *   u = fl(std_beta_j - t)
 *   a = fl(|u| - pen_j)
 *   b = a > 0 ? copysign(a, u) : +0
 *   d = fl(b - eta_old_j)
 *   var_mu[j] = u;  var_gamma[j] = (b != 0) ? 1 : 0;  eta_diff[j] = d;  eta[j] = fl(eta_old_j + d)
 * then the E-step's own update of q over the row's window in index order, q[k] = fma(R[j,k], dq_scale * d, q[k]) (symmetric
 * form: followed by q[j] -= d, e_step.hpp:423-428), and after the block the second pass of the upper form, update_q_factor
 * (e_step.hpp:331-337): q[j] += dq_scale * dot(row(j), eta_diff) with the dot a serial fma chain from 0 in index order.
 * There is no skip branch: a zero d is added like any other and leaves the bits of q alone.  No random numbers, no
 * transcendental function: a sweep is a function of the state and the LD alone, two calls give identical bits.
 *   c_j    VIPRS_FIELD_ENET_MULT (= VIPRS_FIELD_MU_MULT): lassosum's 1 - s
 *   pen_j  VIPRS_FIELD_ENET_PENALTY (= VIPRS_FIELD_SQRT_HALF_VAR_TAU): lambda times an optional per-SNP penalty factor, >= 0
 *   VIPRS_FIELD_U_LOGS is not read.  With a constant c = 1 - s a fixed point of the sweep minimises the objective above.
 * KERNELS.  The panel sweep serves the dense blocks and the band kernel the windowed ones, for fp32, int8 and int16 LD in both
 * forms; the columns of a grid state run as (block, model) items of ONE panel launch, never on the batched matrix-core
 * kernel; `active_model_idx` / `n_active` as in viprs_state_e_step (NULL: every column; ignored for width 1).  The kernel is
 * the same in either math_mode: viprs_plan_last_math_modes reports exact.  Timing goes through the plan's timing record of
 * the sweeps (viprs_plan_last_kernel_ms, viprs_plan_timing_history).
 * REFUSALS, each before any launch: a float64 state VIPRS_EUNSUPPORTED; a mixture state VIPRS_EINVAL; a grid state under a
 * (group, column) mask VIPRS_EUNSUPPORTED; windowed blocks the band kernel cannot take (VIPRS_BAND=0, or a window wider than
 * its q ring) VIPRS_EUNSUPPORTED -- there is no row-by-row kernel for this update.
 *   viprs_enet_route        the route of such a sweep (pure host code; usable without a GPU), the VIPRS_ROUTE_COUNT fields of
 *                           viprs_sweep_route: dense blocks VIPRS_FAMILY_PANEL with model 4, windowed blocks
 *                           VIPRS_FAMILY_BAND with model 3; prologue and events as the spike-and-slab row of viprs_sweep_route
 *                           for width 1 (`grid` == 0) and as its grid row for a grid state.  viprs_sweep_route itself does
 *                           not know the elastic net: its arguments and answers are unchanged
 *   viprs_state_enet_sums   `out`: n rows of VIPRS_N_ENET_SUMS doubles, one per listed column (`cols` NULL: columns
 *                           0 .. n - 1 with n = the state's width; width 1: n = 1):
 *                             [0] max |eta_diff| (fmax: ignores NaN)   [1] sum std_beta eta   [2] sum q eta   [3] sum eta^2
 *                             [4] sum pen |eta|   [5] the number of eta != 0
 *                           every term formed in double from the float32 values (no fma), summed in THE ORDER defined above
 *                           for the rows of a spike-and-slab or grid state (cap 1024 / 256 workgroups).  Synchronous.  With
 *                           viprs_state_set_comm the rows are all-rank sums.  With a constant c = 1 - s the objective above
 *                           is (1 - s) ([2] + [3]) + s [3] - 2 [1] + 2 [4]. */
#define VIPRS_N_ENET_SUMS 6
int viprs_state_enet_sweep(viprs_state* state, double dq_scale, const int32_t* active_model_idx, int n_active, int sync);
int viprs_state_enet_sums(viprs_state* state, int n, const int32_t* cols, double* out);
int viprs_enet_route(int grid, int ld_dtype, int dense, int ragged, int band_ok, int* route);

/* ---- LDpred2: a Gibbs draw where the E-step takes an expectation ---------------------------------------------------------------
 * LDpred2 (Prive, Arbel and Vilhjalmsson 2020; -grid and -auto) samples every effect from its conditional posterior under a
 * point-normal prior (proportion p, heritability h2), SNP after SNP over each LD block with a running q = (R - I) beta.  With
 * C1 = n_j h2 / (m p) its update of SNP j is C2 = C1 / (1 + C1), C3 = C2 (beta_hat_j - q_j), C4 = C2 / n_j,
 * postp = 1 / (1 + (1-p)/p sqrt(1 + C1) exp(-C3^2 / (2 C4))), beta_j = postp > U ? C3 + z sqrt(C4) : 0: the grid-column E-step
 * of viprs_state_e_step with sigma_epsilon = 1, lambda = 0 and tau_beta = m p / h2 -- under these viprs_state_prep_columns
 * writes mu_mult = C2, half_var_tau = 1 / (2 C4) and u_logs = logit(p) - 0.5 log(1 + C1) -- with a draw stored in eta where the
 * E-step stores gamma mu.  The reference has no such model; the definition is this library's own, stated in full.
 * THE DRAWS.  viprs_state_gibbs_draws: for every SNP j of the plan and every listed column g one Philox4x32-10 block (Salmon
 * et al. 2011; multipliers 0xD2511F53 and 0xCD9E8D57, Weyl increments 0x9E3779B9 and 0xBB67AE85, 10 rounds) with
 *   key     = (low 32 bits of seed, high 32 bits of seed)
 *   counter = (j, g, low 32 bits of draw_index, high 32 bits of draw_index)
 * and from its output words x0, x1, x2, every operation separately rounded in float32:
 *   U  = (2 (x0 >> 9) + 1) * 2^-24        exact in float32, strictly inside (0, 1); u1, u2 likewise from x1, x2
 *   z  = sqrtf(-2 logf(u1)) * cospif(2 u2)
 *   noise = z * (1.0f / sqrtf(2.0f * half_var_tau[j, g]))
 * written to two (m, G) float32 buffers of the state (column-major like its fields), allocated by the first Gibbs call and
 * freed with the state.  A draw depends on (seed, draw_index, j, g) alone, never on the launch, the other listed columns or
 * the call that generated it.  logf / cospif are the device library's (a few ulp): U is bit-exact against a host
 * implementation, noise is not (tests/test_gpu_gibbs.py states the bound).
 * THE UPDATE.  Per SNP j in index order and per listed column, from the current q_j, every operation separately rounded in
 * float32, no fused multiply-add, the sigmoid of e_step_grid (e_step.hpp:245-261, :599-635) with glibc's expf:
 *   mu    = fl(mu_mult_j * fl(std_beta_j - q_j))
 *   gamma = sigmoid(fl(u_logs_j + fl(fl(half_var_tau_j * mu) * mu)))
 *   b     = gamma > U_j ? fl(mu + noise_j) : +0                   (strict: gamma == U_j leaves the SNP out)
 *   d     = fl(b - eta_old_j)
 *   var_mu[j] = mu;  var_gamma[j] = gamma;  eta_diff[j] = d;  eta[j] = b
 * then the E-step's own update of q over the row's window, q[k] = fma(R[j,k], dq_scale * d, q[k]) (symmetric form: followed by
 * q[j] -= d), and after the block the second pass of the upper form, as for viprs_state_enet_sweep.  There is no skip branch.
 *   viprs_state_gibbs_sweep   the draws for the listed columns (unless VIPRS_GIBBS_KEEP_DRAWS is set in `flags`: then the
 *                             sweep uses whatever the two buffers hold), then one sweep over every LD block the plan's sweeps
 *                             visit, on an fp32 state of kind VIPRS_MODEL_GRID, width >= 1; `active_model_idx` / `n_active` as
 *                             in viprs_state_e_step (distinct columns; NULL: every column); asynchronous on the plan's stream
 *                             unless `sync` != 0.  The exact arithmetic whatever the plan's math_mode.
 * KERNELS.  The panel sweep serves the dense blocks (model 5) and the band kernel the windowed ones (model 4), for fp32, int8
 * and int16 LD in both forms; the columns run as (block, model) items of ONE panel launch, never on the batched matrix-core
 * kernel.  Sweep timing goes through the plan's timing record (viprs_plan_last_kernel_ms: the draws kernel is outside it);
 * viprs_plan_last_gibbs_draws_ms is the event time of the last draws kernel.
 * REFUSALS, each VIPRS_EINVAL before any launch: a float64 state; a spike-and-slab-kind or mixture state; a grid state under a
 * (group, column) mask; windowed blocks the band kernel cannot take (VIPRS_BAND=0, or a window wider than its q ring);
 * VIPRS_GIBBS_KEEP_DRAWS before the draw buffers exist (no draws call, sweep or upload yet).
 *   viprs_gibbs_route         the route of such a sweep (pure host code; usable without a GPU): dense blocks VIPRS_FAMILY_PANEL
 *                             with model 5, windowed blocks VIPRS_FAMILY_BAND with model 4, prologue and events as the grid row
 *                             of viprs_sweep_route, whose arguments and answers are unchanged
 *   viprs_state_gibbs_upload / _download   one of the state's Gibbs buffers, `which` a viprs_gibbs_buffer: (m, G) column-major,
 *                             float32 (UNIF, NOISE) or float64 (MEAN_SUM); a buffer that does not exist yet is created, zeroed
 *   viprs_state_gibbs_accumulate   mean_sum[j, g] += (double)var_gamma[j, g] * (double)var_mu[j, g] for the listed (distinct)
 *                             columns: the Rao-Blackwellised posterior mean of the draw, summed over sweeps.  Synchronous
 *   viprs_state_gibbs_reset_mean   zeroes mean_sum
 * The per-sweep scalars a sampler needs -- the number of eta != 0, sum q eta, sum eta^2, sum std_beta eta -- are columns
 * [5], [2], [3], [1] of viprs_state_enet_sums.
 * NOT BUILT: LDpred2's `sparse` option; allow_jump_sign / use_MLE / shrink_corr of later bigsnpr versions; float64 and
 * mixture states; several ranks; a math_mode = fast variant. */
enum viprs_gibbs_buffer { VIPRS_GIBBS_UNIF = 0, VIPRS_GIBBS_NOISE = 1, VIPRS_GIBBS_MEAN_SUM = 2, VIPRS_GIBBS_BUFFER_COUNT = 3 };
#define VIPRS_GIBBS_KEEP_DRAWS 1
int viprs_state_gibbs_draws(viprs_state* state, uint64_t seed, uint64_t draw_index, const int32_t* active_model_idx, int n_active);
int viprs_state_gibbs_sweep(viprs_state* state, double dq_scale, const int32_t* active_model_idx, int n_active, uint64_t seed,
                            uint64_t draw_index, int flags, int sync);
int viprs_state_gibbs_upload(viprs_state* state, int which, const void* host);
int viprs_state_gibbs_download(viprs_state* state, int which, void* host);
int viprs_state_gibbs_accumulate(viprs_state* state, const int32_t* active_model_idx, int n_active);
int viprs_state_gibbs_reset_mean(viprs_state* state);
int viprs_gibbs_route(int ld_dtype, int dense, int ragged, int band_ok, int* route);
int viprs_plan_last_gibbs_draws_ms(viprs_plan* plan, double* ms);

/* ---- PRS-CS: continuous-shrinkage Gibbs on the sweep of LDpred2 ----------------------------------------------------------------
 * PRS-CS (Ge et al. 2019) puts the prior beta_j ~ N(0, sigma2 / n * psi_j) on every effect, psi_j ~ Gamma(a, delta_j),
 * delta_j ~ Gamma(b, phi).  Given the other effects the conditional of beta_j is Gaussian with mean
 * psi_j / (1 + psi_j) (beta_hat_j - q_j) and variance sigma2 / (n_j (1 + 1 / psi_j)): what viprs_state_gibbs_sweep draws from
 * mu_mult = psi / (1 + psi), half_var_tau = n_j (1 + 1 / psi) / (2 sigma2) and u_logs = 32 -- the exact sigmoid of x >= 32 is
 * 1.0f in float32 and U < 1, so every SNP is drawn and var_gamma == 1.  The sweep, its kernels and its route are those of the
 * LDpred2 section, untouched.  The calls below are the other half of the sampler: after every sweep a new local scale psi for
 * each (SNP, chain) and the three E-step inputs rewritten from it.  For a = 1, b = 1/2 the draws have closed forms with a
 * fixed number of variates: delta ~ Gamma(3/2) / (psi + phi) with Gamma(3/2) = z^2 / 2 + Exp(1), and psi ~ GIG(1/2, 2 delta,
 * n beta^2 / sigma2), whose reciprocal is inverse-Gaussian (Michael, Schucany and Haas 1976: one normal, one uniform, no
 * rejection loop), written in s = sqrt(b_gig / a_gig) so that beta = 0 needs no special case.  The reference has no such
 * model; the definition is this library's own, stated in full.  All calls: fp32 states of kind VIPRS_MODEL_GRID, one chain per
 * column, `n_j` from viprs_state_set_n_per_snp, lists of DISTINCT columns (NULL: every column).
 * BUFFERS.  Six (m, G) float32 arrays (viprs_cs_buffer; column-major like the fields) in one allocation of the state, made by
 * the first cs call with psi = 1 and the rest zero, freed with the state.  States that never make a cs call do not grow.
 * THE VARIATES.  viprs_state_cs_variates: for every SNP j and every listed column g one Philox4x32-10 block with the constants
 * and the key of viprs_state_gibbs_draws and
 *   counter = (j, g + 2^31, low 32 bits of draw_index, high 32 bits of draw_index)
 * (the tag bit keeps the stream disjoint from the Gibbs draws of the same seed and draw_index), and from its output words
 * x0 .. x3, every operation separately rounded in float32:
 *   ub = (2 (x0 >> 9) + 1) * 2^-24;  u1, u2, u3 likewise from x1, x2, x3
 *   r  = sqrtf(-2 logf(u1))
 *   z1 = r * cospif(2 u2);  z2 = r * sinpif(2 u2)
 *   e  = -logf(u3)
 * written to VIPRS_CS_UB, _Z1, _Z2, _E.  A variate depends on (seed, draw_index, j, g) alone.  ub is bit-exact against a host
 * implementation; z1, z2 and e carry the device library's logf / cospif / sinpif (tests/test_gpu_cs.py states the bounds).
 * THE UPDATE.  viprs_state_cs_update, `params`: n rows (column, sigma2, phi).  Per SNP j and listed column, in float64, every
 * operation separately rounded, no fused multiply-add, from the stored float32 variates, psi_old = VIPRS_CS_PSI[j, g] and
 * eta = VIPRS_FIELD_ETA[j, g]:
 *   g15   = 0.5 z2 z2 + e
 *   delta = g15 / (psi_old + phi)
 *   lam   = 2 delta
 *   s     = |eta| sqrt(n_j / (lam sigma2))
 *   y     = z1 z1
 *   A     = s + (y + sqrt(y (4 lam s + y))) / (2 lam)
 *   psi   = (ub (A + s) <= A) ? A : s s / A
 *   psi   = psi < 2^-40 ? 2^-40 : psi;  psi = psi > psi_max ? psi_max : psi          (comparisons: a NaN stays a NaN)
 *   psi32 = (float)psi;  delta32 = (float)delta;  p = (double)psi32
 *   mu_mult = (float)(p / (1 + p));  half_var_tau = (float)(n_j (1 + 1 / p) / (2 sigma2));  u_logs = 32.0f
 * products associate from the left.  It writes VIPRS_CS_PSI, VIPRS_CS_DELTA and the three fields of the listed columns; other
 * columns keep their bits, buffers and fields alike.  The variates kernel runs first with (seed, draw_index) unless
 * VIPRS_CS_KEEP_VARIATES is set: then the update uses what the buffers hold.  VIPRS_CS_PREPARE_ONLY draws nothing and reads no
 * variate: it rewrites the three fields from the stored psi and the given sigma2 (phi is checked, not used) -- the start of a
 * chain, and the way to change sigma2 alone.  Asynchronous on the plan's stream unless `sync` != 0.  Both kernels are
 * grid-stride walks over the n x m rectangle without LDS or atomics.
 * THE SUMS.  viprs_state_cs_sums, `out`: n rows of VIPRS_N_CS_SUMS doubles, one per listed column (`cols` NULL: columns
 * 0 .. n - 1 with n = the state's width):
 *   [0] sum eta^2 / psi   [1] sum n_j eta^2 / psi   [2] sum delta   [3] sum psi
 * terms formed in double from the float32 values, t = (double)eta * (double)eta / (double)psi, then n_j * t, summed in THE
 * ORDER defined above for the rows of a grid state (cap 256 workgroups), as viprs_state_enet_sums.  Synchronous.
 * REFUSALS, each VIPRS_EINVAL before any launch, outputs untouched: a float64 state; a spike-and-slab-kind or mixture state; a
 * grid state under a (group, column) mask; a state with a communicator (viprs_state_set_comm: several ranks are not built);
 * update and sums without viprs_state_set_n_per_snp; a column out of range or listed twice; sigma2 or phi not positive and
 * finite; psi_max outside (2^-40, inf); an unknown flag; VIPRS_CS_KEEP_VARIATES before the buffers exist; null pointers.  A
 * plan without SNPs returns VIPRS_OK.
 *   viprs_state_cs_upload / _download   one of the six buffers, `which` a viprs_cs_buffer (created if need be)
 *   viprs_plan_last_cs_ms     the event times of the last variates kernel and of the last update kernel (0 for one that has
 *                             not run; VIPRS_EINVAL when neither has)
 * NOT BUILT: a != 1 or b != 1/2; the joint draw of an LD block through its Cholesky factor (the single-site chain has the same
 * stationary distribution); float64 and mixture states; several ranks; a math_mode = fast variant. */
enum viprs_cs_buffer { VIPRS_CS_PSI = 0, VIPRS_CS_DELTA = 1, VIPRS_CS_UB = 2, VIPRS_CS_Z1 = 3, VIPRS_CS_Z2 = 4, VIPRS_CS_E = 5,
                       VIPRS_CS_BUFFER_COUNT = 6 };
#define VIPRS_CS_KEEP_VARIATES 1
#define VIPRS_CS_PREPARE_ONLY 2
#define VIPRS_N_CS_SUMS 4
int viprs_state_cs_variates(viprs_state* state, uint64_t seed, uint64_t draw_index, const int32_t* active_model_idx, int n_active);
int viprs_state_cs_update(viprs_state* state, int n, const double* params, double psi_max, uint64_t seed, uint64_t draw_index,
                          int flags, int sync);
int viprs_state_cs_sums(viprs_state* state, int n, const int32_t* cols, double* out);
int viprs_state_cs_upload(viprs_state* state, int which, const void* host);
int viprs_state_cs_download(viprs_state* state, int which, void* host);
int viprs_plan_last_cs_ms(viprs_plan* plan, double* variates_ms, double* update_ms);

/* ---- PRS-CSx: populations coupled through shared local scales -------------------------------------------------------------------
 * PRS-CSx (Ruan et al. 2022) fits one PRS-CS chain per population k = 0 .. P - 1, each on its own LD panel and summary
 * statistics -- here: each a grid state on a plan of its own, swept by viprs_state_gibbs_sweep exactly as in the PRS-CS section
 * --, and couples them through ONE local scale psi_u per SNP u of the union of the SNP sets: beta_ku ~ N(0, sigma2_k / n_ku *
 * psi_u), psi_u ~ Gamma(1, delta_u), delta_u ~ Gamma(1/2, phi).  With K_u populations carrying SNP u the conditional is
 *   psi_u ~ GIG(p = 1 - K_u / 2, 2 delta_u, B_u),  B_u = sum_k n_ku beta_ku^2 / sigma2_k
 * (density proportional to x^(p - 1) exp(-(a x + b / x) / 2)).  K_u = 1 is the index 1/2 of the PRS-CS section and keeps its
 * closed form; K_u >= 2 (index 0, -1/2, -1, ...) is drawn by the rejection sampler of Devroye (2014) for the log-concave density
 * of log X, the algorithm of PRS-CS's gigrnd.  A viprs_csx handle holds the map from union SNPs to the rows of the P states,
 * the shared psi and delta and the attempt counts; one call per iteration gathers eta from the P states, draws, and scatters
 * the three sweep inputs back.  The reference has no such model; the definition is this library's own, stated in full.
 * THE HANDLE.  viprs_csx_create: `states`, n_pop fp32 states of kind VIPRS_MODEL_GRID of one common width G on one device, each
 * after viprs_state_set_n_per_snp; `row_of`, n_pop x m_union row-major: the row of union SNP u in the plan of population k, or -1.
 * The handle owns the uploaded map, the shared (m_union, G) float32 psi (1) and delta (0), column-major, the (m_union, G) uint8
 * attempt counts (0) and a counter of capped draws; it creates the cs buffers of every state (viprs_cs_buffer).  The states
 * stay the caller's and must outlive the handle.  The kernels run on the stream of population 0's plan.
 * THE UPDATE.  viprs_csx_update, `params`: n rows (column, phi, sigma2_0 .. sigma2_{P-1}).  Per union SNP u and listed column g, in
 * float64, every operation separately rounded, no fused multiply-add, products and sums associate from the left:
 *   1. ub, z1, z2, e: the float32 variates of viprs_state_cs_variates with j = u, counter = (u, g + 2^31, low 32 bits of
 *      draw_index, high 32 bits of draw_index); psi_old = the shared psi[u, g];
 *        g15 = 0.5 z2 z2 + e;  delta = g15 / (psi_old + phi);  lam = 2 delta
 *   2. B = 0; for k ascending over the populations with r = row_of[k][u] >= 0:  B = B + n_kr eta_kr eta_kr / sigma2_k
 *      (eta_kr = (double)VIPRS_FIELD_ETA[r, g] of state k); K = the number of such populations.
 *   3. K == 1: with eta, n, sigma2 of the one carrying population, s = |eta| sqrt(n / (lam sigma2)); y = z1 z1;
 *        A = s + (y + sqrt(y (4 lam s + y))) / (2 lam);  psi = (ub (A + s) <= A) ? A : s s / A
 *      K >= 2 and B == 0: psi = 2^-40 (the conditional is improper; nothing is drawn, 0 attempts).
 *      K >= 2 otherwise, with psi(x) = -alpha (cosh(x) - 1) - lambda (exp(x) - x - 1), dpsi(x) = -alpha sinh(x) - lambda (exp(x) - 1)
 *      and C1 = cosh(1), E1 = exp(1), EM1 = exp(-1) rounded to float64:
 *        lambda = 0.5 K - 1;  omega = sqrt(lam B);  alpha = sqrt(omega omega + lambda lambda) - lambda
 *        x = alpha (C1 - 1) + lambda (E1 - 1 - 1);   t = 1 if 0.5 <= x <= 2;  sqrt(2 / (alpha + lambda)) if x > 2;
 *                                                    log(4 / (alpha + 2 lambda)) if x < 0.5
 *        x = alpha (C1 - 1) + lambda EM1;            s = 1 if 0.5 <= x <= 2;  sqrt(4 / (alpha C1 + lambda)) if x > 2;  if x < 0.5:
 *                                                    ia = 1 / alpha;  s = log(1 + ia + sqrt(ia ia + 2 ia));
 *                                                    and only if lambda > 0:  s = fmin(1 / lambda, s)
 *        (lambda = 0, two populations, takes the log branch alone: no 1 / lambda is formed)
 *        eta' = -psi(t);  zeta = -dpsi(t);  theta = -psi(-s);  xi = dpsi(-s);  pe = 1 / xi;  re = 1 / zeta
 *        td = t - re eta';  sd = s - pe theta;  q = td + sd;  norm = pe + q + re;  cut1 = q / norm;  cut2 = (q + re) / norm
 *      attempt a = 0, 1, ..: one Philox4x32-10 block, the key of the variates,
 *        counter = (u, g + 2^31 + (a + 1) 2^16, low 32 bits of draw_index, high 32 bits of draw_index)
 *      (bits 16..21 of the second word: disjoint from the variates, whose a + 1 is 0, and from the Gibbs draws; hence G < 2^16);
 *      U, V, W = (double) of the open-unit float32 uniforms (2 (x_i >> 9) + 1) * 2^-24 of its words x0, x1, x2;
 *        x = -sd + q V if U < cut1;  td - re log(V) if U < cut2;  -sd + pe log(V) otherwise
 *        gx = exp(-eta' - zeta (x - t)) if x > td;  exp(-theta + xi (x + s)) if x < -sd;  1 otherwise
 *        accept when W gx <= exp(psi(x))
 *      THE ATTEMPT CAP IS 32 (VIPRS_CSX_MAX_ATTEMPTS): a draw still rejected at a = 31 keeps that proposal and adds one to the
 *      handle's counter of capped draws (a global atomic add).  The measured worst rejection share is 0.177 (p = 0, omega = 1):
 *      0.2^32 is about 4e-23 per draw.  A NaN never accepts: it ends at the cap and stays a NaN.  Then
 *        lo = lambda / omega;  psi = exp(x) (lo + sqrt(1 + lo lo));  if K > 2 (p < 0): psi = 1 / psi;  psi = psi / sqrt(lam / B)
 *      The attempt count of (u, g) is a + 1 of the last attempt, 0 where nothing was drawn.  exp, log, cosh, sinh are the device
 *      library's float64 functions: against a host implementation psi agrees to one float32 ulp, not bit for bit.
 *   4. psi = psi < 2^-40 ? 2^-40 : psi;  psi = psi > psi_max ? psi_max : psi          (comparisons: a NaN stays a NaN)
 *      psi32 = (float)psi;  delta32 = (float)delta, stored in the shared psi and delta.
 *   5. for every carrying population k at its row r: VIPRS_CS_PSI[r, g] = psi32, VIPRS_CS_DELTA[r, g] = delta32, the four
 *      variates into VIPRS_CS_UB, _Z1, _Z2, _E, and with p = (double)psi32
 *        mu_mult = (float)(p / (1 + p));  half_var_tau = (float)(n_kr (1 + 1 / p) / (2 sigma2_k));  u_logs = 32.0f
 *      so that the unchanged viprs_state_cs_sums of state k yields that population's sum eta^2 / psi and sum n eta^2 / psi.
 * Columns not listed keep their bits, in the handle and in every state.  A handle over one population with the identity map
 * gives the bits of viprs_state_cs_update, every buffer and field.  Flags, those of viprs_state_cs_update:
 * VIPRS_CS_KEEP_VARIATES reads ub, z1, z2, e from the cs buffers of the first carrying population instead of drawing them (the
 * four closed-form variates only: the attempts of the sampler are always drawn); VIPRS_CS_PREPARE_ONLY draws nothing and
 * rewrites step 5 (psi, delta, the three fields; not the variates) from the stored shared psi and delta.
 * ORDER ACROSS STREAMS.  The P states sit on P plans with P streams.  The update waits for an event recorded on every member
 * stream at the call, and every member stream waits for the event recorded behind the update kernel before anything it is
 * given later: a sweep enqueued before the call is finished before the update reads its eta, a sweep enqueued after the call
 * reads the new inputs.  Asynchronous unless `sync` != 0.  One grid-stride walk over the n x m_union rectangle, at most 8192
 * workgroups of 256, no LDS; the rejection loop is per lane.
 * THE SUMS.  viprs_csx_sums, `out`: n rows of VIPRS_N_CSX_SUMS doubles, one per listed column (`cols` NULL: every column, n = G):
 *   [0] sum delta   [1] sum psi      over the union, the shared float32 values converted to double,
 * summed in THE ORDER defined above for the rows of a grid state (cap 256 workgroups).  Synchronous.
 * REFUSALS of viprs_csx_create, each VIPRS_EINVAL before any allocation: n_pop outside 1..8; a state that is not an fp32
 * VIPRS_MODEL_GRID state; states of different widths; states on different devices; a state under a (group, column) mask or with
 * a communicator; a state without viprs_state_set_n_per_snp; a state listed twice; a union row carried by no population; a row
 * index out of range or listed twice within one population; G >= 2^16; m_union >= 2^32; null pointers.  Of the other calls,
 * before any launch: a null handle; a column out of range or listed twice; phi or a sigma2 not positive and finite; psi_max
 * outside (2^-40, inf); an unknown flag; a bad buffer code; null pointers.
 *   viprs_csx_upload / _download   the shared psi or delta (float32) or the attempt counts (uint8), `which` a viprs_csx_buffer
 *   viprs_csx_last                 the event time of the last update kernel and how many of its draws ended at the attempt cap
 * NOT BUILT: a != 1 or b != 1/2; joint-block draws; float64 states; several ranks; a math_mode = fast variant; populations on
 * different devices. */
typedef struct viprs_csx viprs_csx;
enum viprs_csx_buffer { VIPRS_CSX_PSI = 0, VIPRS_CSX_DELTA = 1, VIPRS_CSX_ATTEMPTS = 2, VIPRS_CSX_BUFFER_COUNT = 3 };
#define VIPRS_CSX_MAX_POP 8
#define VIPRS_CSX_MAX_ATTEMPTS 32
#define VIPRS_N_CSX_SUMS 2
int viprs_csx_create(viprs_csx** out, int n_pop, viprs_state* const* states, int64_t m_union, const int64_t* row_of);
int viprs_csx_destroy(viprs_csx* x);
int viprs_csx_update(viprs_csx* x, int n, const double* params, double psi_max, uint64_t seed, uint64_t draw_index, int flags,
                     int sync);
int viprs_csx_sums(viprs_csx* x, int n, const int32_t* cols, double* out);
int viprs_csx_upload(viprs_csx* x, int which, const void* host);
int viprs_csx_download(viprs_csx* x, int which, void* host);
int viprs_csx_last(viprs_csx* x, double* ms, int64_t* n_capped);

/* ---- SBayesR: a mixture Gibbs draw where the mixture E-step takes an expectation ---------------------------------------------
 * SBayesR (Lloyd-Jones et al. 2019; GCTB --sbayes R) samples every effect from its conditional posterior under a finite mixture
 * of normals with a point mass at zero: component k = 1..K has prior variance gamma_k sigma2_beta and weight pi_k, component 0
 * is the null with weight pi_0; sigma2_e is the residual variance.  With r_j = std_beta_j - q_j and
 * C_jk = n_j + sigma2_e / (gamma_k sigma2_beta) the conditional of SNP j picks component k with log-weight
 * log pi_k - 0.5 log(1 + n_j gamma_k sigma2_beta / sigma2_e) + n_j^2 r_j^2 / (2 C_jk sigma2_e) (the null: log pi_0) and then
 * draws from N(n_j r_j / C_jk, sigma2_e / C_jk): the mixture E-step of viprs_state_e_step under lambda = 0,
 * tau_beta[k] = 1 / (gamma_k sigma2_beta), sigma_epsilon = sigma2_e, logit_pi[k] = log pi_k and log_null_pi = log pi_0 -- under
 * these viprs_state_prep_mixture writes mu_mult = n_j / C_jk, sqrt_half_var_tau = sqrt(C_jk / (2 sigma2_e)) and u_logs = the first
 * two terms of the log-weight -- with a draw stored in eta where the E-step stores sum_k gamma_k mu_k.  The reference has no such
 * model; the definition is this library's own, stated in full.  All calls: fp32 states of kind VIPRS_MODEL_MIXTURE, K <= 4,
 * `n_j` from viprs_state_set_n_per_snp.
 * BUFFERS.  U, z (float32) and k* (int32), each (m,), in ONE allocation of the state, made by the first SBayesR call (zeros) and
 * freed with the state; mean_sum and pip_sum, (m,) float64, created on first use.  Other states do not grow.
 * THE DRAWS.  viprs_state_bayesr_draws: for every SNP j one Philox4x32-10 block with the constants and the key of
 * viprs_state_gibbs_draws and
 *   counter = (j, 2^30, low 32 bits of draw_index, high 32 bits of draw_index)
 * (the tag keeps the stream disjoint from the Gibbs draws, whose second word is a column < 2^30, and from the PRS-CS variates,
 * whose second word has bit 31 set), and from its output words x0, x1, x2, every operation separately rounded in float32:
 *   U = (2 (x0 >> 9) + 1) * 2^-24;  u1, u2 likewise from x1, x2
 *   z = sqrtf(-2 logf(u1)) * cospif(2 u2)
 * U is bit-exact against a host implementation; z carries the device library's logf / cospif (tests/test_gpu_bayesr.py states
 * the bound).
 * THE UPDATE.  Per SNP j in index order, from the current q_j, every operation separately rounded in float32, fused
 * multiply-add only where written, glibc's expf, as e_step_mixture (e_step.hpp:496-537):
 *   r = fl(std_beta_j - q_j)
 *   mu_k = fl(mu_mult_jk * r);  t_k = fl(sqrt_half_var_tau_jk * mu_k);  u_k = fma(t_k, t_k, u_logs_jk)              k = 1..K
 *   mx = max(log_null_pi_j, u_1, .., u_K)
 *   e_k = expf(u_k - mx);  ssum = ((0 + e_1) + .. + e_K) + expf(log_null_pi_j - mx)            (the null term last)
 *   gamma_k = fl(e_k / ssum)
 *   sd_k = fl(0x1.6a09e6p-1f / sqrt_half_var_tau_jk);  n_k = fl(z_j * sd_k)      (0x1.6a09e6p-1f = float32(1 / sqrt 2))
 *   c_1 = gamma_1;  c_k = fl(c_{k-1} + gamma_k)
 *   k* = the smallest k in 1..K with U_j < c_k (strict), 0 if there is none
 *   b = k* ? fl(mu_{k*} + n_{k*}) : +0
 *   d = fl(b - eta_old_j)
 *   var_mu[j, k] = mu_k;  var_gamma[j, k] = gamma_k;  eta_diff[j] = d;  eta[j] = b;  kstar[j] = k*
 * then the E-step's own update of q over the row's window, q[i] = fma(R[j,i], dq_scale * d, q[i]) (symmetric form: followed by
 * q[j] -= d), and after the block the second pass of the upper form, as for viprs_state_enet_sweep.  There is no skip branch.
 *   viprs_state_bayesr_sweep  the draws (unless VIPRS_BAYESR_KEEP_DRAWS is set in `flags`: then the sweep uses whatever U and z
 *                             hold), then one sweep over every LD block the plan's sweeps visit; asynchronous on the plan's
 *                             stream unless `sync` != 0.  The exact arithmetic whatever the plan's math_mode.
 * KERNELS.  The panel sweep serves the dense blocks (model 6), one lane per SNP, for fp32, int8 and int16 LD in both forms; the
 * band kernel serves the windowed ones (model 5) for the same LD types in the symmetric form only.  Sweep timing goes through
 * the plan's timing record (the draws kernel is outside it); viprs_plan_last_bayesr_draws_ms is the event time of the last draws
 * kernel.
 *   viprs_bayesr_route        the route of such a sweep (pure host code; usable without a GPU): prologue and events as the
 *                             mixture row of viprs_sweep_route, whose arguments and answers are unchanged
 * THE SUMS.  viprs_state_bayesr_sums, `out`: 2 K + 4 doubles,
 *   [0 .. K] the number of SNPs with k* = 0 .. K   [K + k] sum eta_j^2 over k*_j = k, k = 1 .. K
 *   [2K + 1] sum q eta   [2K + 2] sum eta^2   [2K + 3] sum std_beta eta
 * (viprs_state_enet_sums refuses a mixture state, so its three sums travel here), every term formed in double from the float32
 * values (no fma), summed in THE ORDER of viprs_state_enet_sums for the row of a spike-and-slab state (cap 1024 workgroups; no
 * maximum among them).  Synchronous.
 *   viprs_state_bayesr_accumulate   mean_sum[j] += ((0 + g_1 m_1) + .. + g_K m_K) and pip_sum[j] += ((0 + g_1) + .. + g_K), with
 *                             g_k = (double)var_gamma[j, k], m_k = (double)var_mu[j, k]: the Rao-Blackwellised posterior mean
 *                             of the draw and its probability 1 - gamma_0 of being non-zero, summed over sweeps.  Asynchronous
 *   viprs_state_bayesr_reset_mean   zeroes both
 *   viprs_state_bayesr_upload / _download   one of the five buffers, `which` a viprs_bayesr_buffer (created, zeroed, if need be)
 * REFUSALS, each VIPRS_EINVAL before any launch: a float64 state; a spike-and-slab or grid state; K > 4; a state with SNP groups
 * or a communicator; no viprs_state_set_n_per_snp; windowed blocks the band kernel cannot take (VIPRS_BAND=0, a window wider than
 * its q ring, or an upper-form plan); an LD element type outside fp32 / int8 / int16; VIPRS_BAYESR_KEEP_DRAWS, or the sums,
 * before the draw buffers exist; an unknown flag; null pointers.  A plan without SNPs returns VIPRS_OK.
 * NOT BUILT: GCTB's --rsq / --p-value filters and its robust parameterisation; K > 4; float64 states; several ranks; a
 * math_mode = fast variant; row-by-row kernels; windowed blocks in the upper form; per-chromosome hyper-parameters. */
enum viprs_bayesr_buffer { VIPRS_BAYESR_UNIF = 0, VIPRS_BAYESR_Z = 1, VIPRS_BAYESR_KSTAR = 2, VIPRS_BAYESR_MEAN_SUM = 3,
                           VIPRS_BAYESR_PIP_SUM = 4, VIPRS_BAYESR_BUFFER_COUNT = 5 };
#define VIPRS_BAYESR_KEEP_DRAWS 1
#define VIPRS_BAYESR_MAX_K 4
int viprs_state_bayesr_draws(viprs_state* state, uint64_t seed, uint64_t draw_index);
int viprs_state_bayesr_sweep(viprs_state* state, double dq_scale, uint64_t seed, uint64_t draw_index, int flags, int sync);
int viprs_state_bayesr_sums(viprs_state* state, double* out);
int viprs_state_bayesr_accumulate(viprs_state* state);
int viprs_state_bayesr_reset_mean(viprs_state* state);
int viprs_state_bayesr_upload(viprs_state* state, int which, const void* host);
int viprs_state_bayesr_download(viprs_state* state, int which, void* host);
int viprs_bayesr_route(int ld_dtype, int dense, int ragged, int band_ok, int* route);
int viprs_plan_last_bayesr_draws_ms(viprs_plan* plan, double* ms);

/* ---- LD product: Y = R B over EVERY block of a plan -------------------------------------------------------------------
 * What the reference computes with `ld.dot(B)`: the pseudo-validation metrics against a validation LD panel
 * (viprs/eval/pseudo_metrics.py:122-127: R_val B for all grid models at once) and q + beta = R beta for effects that were
 * not fitted in this process (BayesPRSModel.py:397-404).  `B` and `Y` are (m, n_cols), column-major like the grid arrays
 * (n_cols = 1: plain vectors), in the state precision `float_dtype`.
 *   S[j, g] = sum over the OFF-DIAGONAL entries (j, i) of row j of the symmetric matrix the plan stands for of r_ji B[i, g]
 *             (symmetric form: the stored diagonal entry is skipped; upper form: the stored row (j, j + len_j] and the
 *             transposed entries (i, j) of the rows i < j that reach j -- the R of q = (R - I) eta, e_step.hpp:410-428);
 *             integer LD: r_ji is the stored integer
 *   Y = fl(fl(dq_scale) * S)            include_diagonal == 0   (the q of a given eta)
 *   Y = fl(fl(fl(dq_scale) * S) + B)    include_diagonal != 0   (unit diagonal: R B)
 * dq_scale is rounded to the state precision first; the multiply and the add are two separately rounded operations.
 * viprs_plan_set_active_blocks does NOT filter the product.  No floating-point atomics.
 * THE ORDER.  The entries of row j lie in a window of W consecutive columns starting at c_lo: a dense block's rows take
 * the block (W = its size); a windowed row of the symmetric form its stored window; of the upper form the columns from the
 * lowest row that reaches j to j + len_j.  W = L + 1 for a row of L off-diagonal entries whose window has no gaps (always,
 * for dense blocks and for symmetric windows).  With V = 16 / sizeof(LD element) (4 for fp32 LD, 8 for int16, 16 for int8),
 * the entry at column c_lo + e goes to accumulator e % V of lane (e / V) % 64; a lane adds its entries in ascending e,
 * each by one fused multiply-add in the state precision (float32 state: fp32; float64 state: float64; the LD element is
 * converted to the state precision first, exactly for int8 / int16 / fp32 LD); the diagonal and columns without an entry
 * add an exact zero.  A lane's V accumulators are then summed in a binary tree, then the 64 lanes in a binary tree.  The
 * longest path of a row therefore has
 *   D(L) = ceil((L + 1) / (64 V)) + log2(V) + 6   additions     (W in place of L + 1 for a window with gaps),
 * every S is within eps_T * D(L) * sum |r_ji B[i, g]| of the exact sum, and it depends on nothing but the row's entries
 * and column g of B: not on the other columns or their number, not on which storage of the upper form the dense blocks are
 * in, not on the active blocks, not on timing.  Two calls give identical bits.
 *   viprs_plan_dot          host buffers in and out, on the plan's stream, synchronous
 *   viprs_state_dot         B = a resident field of `state`: VIPRS_FIELD_ETA only ((m,) for spike-and-slab and mixture
 *                           states, (m, G) for grid states); `y_host` receives m x n_cols results, no input is moved
 *   viprs_plan_last_dot_ms  HIP-event time of the kernels of the last product on this plan; the sweeps' timing ring
 *                           (viprs_plan_last_kernel_ms, viprs_plan_timing_history) never sees a product
 * Bad dtype code, n_cols < 1, a field other than VIPRS_FIELD_ETA, null pointers: VIPRS_EINVAL before any launch, `y_host`
 * untouched.  An empty plan returns VIPRS_OK.  Upper form: the product reads the dense blocks in whichever storage the last
 * sweep left them (the fp32 sweeps' mirrored squares as whole rows; the float64 sweeps' zero lower triangle by gathering
 * the entries left of the diagonal from the column above it), so a product between EM rounds converts nothing; only a plan
 * that has not been swept yet is mirrored once. */
int viprs_plan_dot(viprs_plan* plan, int float_dtype, int n_cols, const void* b_host, void* y_host,
                   double dq_scale, int include_diagonal);
int viprs_state_dot(viprs_state* state, int field, double dq_scale, int include_diagonal, void* y_host);
int viprs_plan_last_dot_ms(viprs_plan* plan, double* ms);

/* ---- LD scores: l[j, g] = sum_k A[k, g] r_jk^2 over EVERY block of a plan ----------------------------------------------
 * What the reference gets from magenpy's LD layer (`compute_ld_scores`, with `annotation_matrix` for the stratified
 * scores) and feeds to `magenpy.stats.h2.ldsc.simple_ldsc` (viprs/model/LDPredInf.py:32-33, VIPRS.py:279-292).  magenpy is
 * not part of the reference tree: the definition below is this library's own, stated in full.
 * `a_host` and `scores_host` are (m, n_cols), column-major, in the state precision `float_dtype`; `a_host == NULL` means ONE
 * column of ones (n_cols must be 1): that path loads no weights at all.  `corr_host` is (m,) doubles or NULL.
 * Per row j and column g, over the OFF-DIAGONAL entries (j, i) of row j -- the entry set of viprs_plan_dot: a stored zero
 * is an entry, the gaps of a window and the diagonal are not --
 *   S2[j, g] = sum p_ji A[i, g]     x = T(stored element) (exact for int8 / int16 / fp32 LD), p = fl(x x); every term enters
 *                                   by ONE fused multiply-add fma(p, A[i, g], acc) in the state precision T
 *   S0[j, g] = sum A[i, g]          plain additions into a second accumulator
 * both in THE ORDER of viprs_plan_dot: entry e of the row's window to accumulator e % V of lane (e / V) % 64 in ascending
 * e, then the binary tree over V, then the xor butterfly over the 64 lanes; the diagonal and the gaps add an exact zero to
 * both.  (Unit weights: S2 = sum p in that order, S0 = the number of entries of the row.)  Then, every operation
 * separately rounded in T, no contraction:
 *   d = fl(dq_scale);  d2 = fl(d d);  U = fl(d2 S2)
 *   corr_host == NULL:  score = fl(U + A[j, g])
 *   corr_host != NULL:  c = fl(corr[j]);  score = fl(fl(U + fl(c fl(U - S0))) + A[j, g])
 * The corrected form is sum_k a_k (r^2 - (1 - r^2) c) with c_j = 1 / (n_LD - 2), the adjusted r^2 of LD-score regression,
 * rearranged so that the two sums suffice; the diagonal contributes A[j, g] in both forms (r_jj = 1, its correction is 0).
 * int16 squares above 2^24 round in a float32 state: p = fl(x x) is the definition.
 * ROUNDING.  Every S2 is within eps_T (D(L) + 1) sum p |A| of the exact sum of the squares (D(L) as defined for the
 * product; the + 1 is the rounding of p), every S0 within eps_T D(L) sum |A| of its exact sum.  A column's result depends
 * on nothing but the row's entries and that column: not on the other columns or their number, not on which storage of the
 * upper form the dense blocks are in, not on the active blocks (viprs_plan_set_active_blocks does NOT filter the call), not
 * on timing.  Two calls give identical bits.  No LDS, no atomics.
 * On the plan's stream, synchronous; an upper-form plan that has not been swept yet is mirrored once, as for the product.
 * Bad dtype code, n_cols < 1, a_host == NULL with n_cols != 1, a null plan or a null output: VIPRS_EINVAL before any launch,
 * `scores_host` untouched.  An empty plan returns VIPRS_OK.
 *   viprs_plan_last_ld_score_ms  HIP-event time of the kernels of the last call on this plan; the sweeps' timing ring never
 *                                sees the call */
int viprs_plan_ld_scores(viprs_plan* plan, int float_dtype, int n_cols, const void* a_host, const double* corr_host,
                         void* scores_host, double dq_scale);
int viprs_plan_last_ld_score_ms(viprs_plan* plan, double* ms);

/* ---- greedy LD clumping: index_of[k, g] = the index SNP that claimed SNP k under threshold g ----------------------------
 * The primitive of clumping + thresholding (C+T / P+T): walk the SNPs from the most significant down, make each unclaimed
 * SNP an index SNP, and assign every SNP in LD with it above a threshold to its clump.  With the SNPs in natural order the
 * same operation is LD pruning.  The definition is this library's own, stated in full.
 *   order_host     n_order DISTINCT SNP indices in processing order, most significant first; n_order may be 0
 *   member_host    (m,) bytes, non-zero = the SNP may belong to a clump; NULL = every SNP may.  Every SNP of `order` must be
 *                  a member
 *   r2_host        n_cols thresholds, 1 <= n_cols <= 32, each finite and >= 0
 *   index_of_host  (m, n_cols) int32, column-major like every multi-column array of this header
 * ENTRIES.  The entries of row j are exactly the entry set of viprs_plan_dot: the off-diagonal entries of the symmetric
 * matrix the plan stands for; a stored zero is an entry, the gaps of a window and the diagonal are not; in the upper form
 * the transposed entries (i, j) of the rows i < j that reach j belong to row j.
 * PASS TEST.  An entry with stored element x passes column g iff (double)x * (double)x >= thr[g].  The host computes
 * s2 = dq_scale * dq_scale and thr[g] = r2[g] / s2, two double operations.  The product is exact for int8, int16, int32
 * and fp32 LD; for int64 and f64 LD it is rounded once, deterministically.
 * PER COLUMN g, independently of the other columns:
 *   1. avail = member, index_of[:, g] = -1
 *   2. take j = order[0], order[1], ... in turn
 *   3. if !avail[j], skip j
 *   4. otherwise index_of[j, g] = j and avail[j] = 0
 *   5. for every entry (j, k) with avail[k] that passes column g: index_of[k, g] = j and avail[k] = 0
 * A column's result depends only on the plan's entries, `order`, `member` and that column's threshold: not on the other
 * columns, not on which storage of the upper form the dense blocks are in, not on the active blocks
 * (viprs_plan_set_active_blocks does NOT filter the call), not on timing.  The results are integers: two calls give
 * identical values.  One workgroup per LD block (LD blocks share no entry), no atomics of any kind, no waiting on another
 * workgroup.  On the plan's stream, synchronous; an upper-form plan that has not been swept yet is mirrored once, as for the
 * product.  An empty plan returns VIPRS_OK.
 * A null plan, output or r2, n_cols outside 1..32, a negative or non-finite threshold, dq_scale not finite or <= 0, an
 * `order` entry out of range, repeated or not a member: VIPRS_EINVAL before any launch, `index_of_host` untouched.
 *   viprs_plan_last_clump_ms  HIP-event time of the kernels of the last call on this plan; the sweeps' timing ring never
 *                             sees the call */
int viprs_plan_clump(viprs_plan* plan, int64_t n_order, const int32_t* order_host, const uint8_t* member_host,
                     int n_cols, const double* r2_host, double dq_scale, int32_t* index_of_host);
int viprs_plan_last_clump_ms(viprs_plan* plan, double* ms);

/* ---- ridge solve: the LDPred-inf estimate, one MINRES per LD block -----------------------------------------------------
 * Solves (R + diag(shift)) x = b, independently for every LD block of the plan (blocks as viprs_plan_get_blocks lists
 * them, SNP order), by MINRES (Paige & Saunders 1975), x0 = 0 or the caller's. R = unit diagonal + dq_scale * stored
 * off-diagonal entries: exactly the matrix of viprs_plan_dot(..., include_diagonal = 1).  What the reference's
 * LDPredInf.fit() (viprs/model/LDPredInf.py:43-114) asks of scipy's minres over ONE assembled block-diagonal matrix; the
 * system decouples block by block, so every block has its own scalars, its own stopping decision and its own iteration
 * count, and all blocks advance in lock step: one LD product and one fused kernel per iteration on the plan's stream.
 *   b, x0, x   (m,) in the state precision `float_dtype`; shift (m,) double, rounded to the state precision
 *              (y_j = (R v)_j + fl(shift_j) v_j); x0 may be NULL
 *   per block  r1 = y = b - A x0, beta1 = ||y||; every iteration: v = y / beta, y = A v, (itn >= 2) y -= (beta / oldb) r1,
 *              alfa = v.y, y -= (alfa / beta) r2, r1 <- r2 <- y, oldb <- beta, beta = ||y||, the Givens rotation of
 *              (oldeps, delta, gbar, epsln, dbar, gamma, cs, sn, phi, phibar), w = (v - oldeps w1 - delta w2) / gamma,
 *              x += phi w; the block stops when phibar <= rtol ||b|| (||b|| = beta1 unless x0 is given) or beta == 0
 *   precision  vectors and the product in the state precision; every scalar and every dot product in double
 *   order      dot products: 16-byte chunks of the block dealt to 256 threads in turn, per-thread partial sums in ascending
 *              order, an xor butterfly over the 64 lanes, the wavefronts in order -- a function of the block's size alone;
 *              a chunk is 16 bytes of the STATE precision: 16 / sizeof(T) consecutive elements (4 float32, 2 float64) in
 *              every dot product of a solve, whatever the type of the values summed;
 *              no floating-point atomics.  A block's result does not depend on the other blocks of the plan, on
 *              `check_every` or on timing; two calls give identical bits
 *   outputs    block_iters / block_relres / block_status (each may be NULL), one entry per block: iterations done, the
 *              solver's own estimate phibar / ||b|| of the relative residual, and 0 converged, 1 stopped at max_iter,
 *              2 zero right-hand side (x = 0, 0 iterations)
 *   host loop  the number of blocks still running is read back every `check_every` iterations (the only synchronisation
 *              inside the loop); a block whose status is final is frozen: later launches leave it unchanged
 * viprs_plan_set_active_blocks does NOT filter the solve.  The workspace lives on the plan and is reused.  The dense blocks of
 * the upper form are read in whichever storage the last sweep left them, as by the product.
 * Bad dtype code, rtol <= 0, max_iter < 1, check_every < 1, a null plan / b / shift / x: VIPRS_EINVAL before any launch,
 * outputs untouched.  An empty plan returns VIPRS_OK.
 *   viprs_plan_last_solve_ms  HIP-event time from the first to the last kernel of the last solve on this plan (the
 *                             read-backs of the loop included) and the iterations it launched */
int viprs_plan_solve_ridge(viprs_plan* plan, int float_dtype, const void* b_host, const double* shift_host,
                           const void* x0_host /* nullable */, void* x_host, double dq_scale, double rtol,
                           int max_iter, int check_every,
                           int32_t* block_iters, double* block_relres, int32_t* block_status /* each nullable */);
int viprs_plan_last_solve_ms(viprs_plan* plan, double* total_ms, int* iterations);

/* ---- extremal eigenvalues: one Lanczos recurrence per LD block ----------------------------------------------------------
 * The smallest and the largest eigenvalue of A = unit diagonal + dq_scale * stored off-diagonal entries -- exactly the matrix
 * of viprs_plan_dot(..., include_diagonal = 1) -- independently for every LD block of the plan (blocks as
 * viprs_plan_get_blocks lists them, SNP order).  What `lambda_min='infer'` needs (viprs/model/VIPRS.py:174-191 asks the LD
 * matrix for get_lambda_min(min_max_ratio), which magenpy answers from extremal eigenvalues it computed per block with ARPACK
 * when the store was built); here every block has its own scalars, its own stopping decision and its own iteration count,
 * and all blocks advance in lock step: one LD product and one fused kernel per iteration on the plan's stream.
 *   start      a function of the index i inside the block only: h = the splitmix64 finaliser of (i + 1) * 0x9E3779B97F4A7C15
 *              (mod 2^64), u_i = (h >> 40) * 2^-24 - 0.5 + 2^-25 (an odd multiple of 2^-25: exact in float32, never zero),
 *              v = fl(u / ||u||).  Not a constant vector: AR(1) blocks are centrosymmetric and the eigenvector of their
 *              smallest eigenvalue is antisymmetric for even sizes -- a symmetric start vector never sees it
 *   per block  iteration k = 1, 2, ... (beta_1 = 0): w = A v - fl(beta_k) v_prev, alpha_k = v.w, w -= fl(alpha_k) v,
 *              beta_{k+1} = ||w||, v_prev <- v, v <- fl(w / beta_{k+1})
 *   no reorthogonalisation: the extremal Ritz values converge without it, the ghost copies that the loss of orthogonality
 *              brings appear at eigenvalues that have already converged and do no harm at the two ends, and the residual
 *              estimate below stays valid to O(eps ||A||) (Paige 1980)
 *   precision  vectors and the product in the state precision `float_dtype`; every scalar and every dot product in double
 *   order      dot products in the order of the ridge solve above (the norm of the start vector u, whose values are doubles,
 *              included: 16 / sizeof(T) elements to a chunk there too): a function of the block's size alone; no floating-point
 *              atomics.  A block's result does not depend on its place in the plan, on the other blocks or on timing; two
 *              calls give identical bits
 *   stopping   at k = 1, 2, 4, 8, ... and at max_iter the host takes the extreme Ritz pairs (theta, s) of the tridiagonal
 *              T_k (diagonal alpha_1..k, off-diagonal beta_2..k) by the implicit QL iteration, carrying only the last row
 *              of the eigenvector matrix (O(k^2) operations, O(k) memory).  beta_{k+1} |s_k| is the residual norm of the
 *              Ritz vector, an upper bound of the distance from theta to the nearest eigenvalue of A.  A block stops when
 *              both bounds are <= rtol * max(|theta_min|, |theta_max|), or when beta_{k+1} == 0.  k reaching the block's
 *              size does NOT stop it: in finite precision the Ritz values at k = size are not the eigenvalues.  A block
 *              whose status is final is frozen: later launches leave it unchanged
 *   outputs    (each may be NULL) one entry per block: lam_min / lam_max, resid_min / resid_max (the two bounds, absolute),
 *              iters, status: 0 converged, 1 stopped at max_iter (the Ritz values and bounds of T_max_iter are returned).
 *              A 1-SNP block gives 1, 1, 0, 0 after 1 iteration
 * viprs_plan_set_active_blocks does NOT filter the computation.  The workspace (three vectors, 16 * max_iter bytes per block)
 * lives on the plan and is reused.  The dense blocks of the upper form are read in whichever storage the last sweep left
 * them, as by the product.
 * Bad dtype code, rtol <= 0, max_iter < 1, a null plan: VIPRS_EINVAL before any launch, outputs untouched.  An empty plan
 * returns VIPRS_OK.
 *   viprs_plan_last_spectrum_ms  HIP-event time from the first to the last kernel of the last call on this plan (the checks
 *                                of the stopping rule included), the iterations it launched, and (nullable) the host's
 *                                time inside those checks
 *   viprs_tridiagonal_extremes   the stopping rule's host routine on its own, no device involved: diagonal alpha[0..k-1],
 *                                off-diagonal beta[0..k-2]; out = {theta_min, theta_max, |s_k| of theta_min, |s_k| of
 *                                theta_max}.  k < 1 or a null pointer: VIPRS_EINVAL */
int viprs_plan_extremal_eigenvalues(viprs_plan* plan, int float_dtype, double dq_scale, double rtol, int max_iter,
                                    double* lam_min, double* lam_max, double* resid_min, double* resid_max,
                                    int32_t* block_iters, int32_t* block_status /* each nullable */);
int viprs_plan_last_spectrum_ms(viprs_plan* plan, double* total_ms, int* iterations, double* host_ms /* nullable */);
int viprs_tridiagonal_extremes(int k, const double* alpha, const double* beta, double* out);

/* ---- SuSiE fine-mapping: L single effects per LD block, lock-step single-effect updates -----------------------------------
 * SuSiE-RSS (Wang et al. 2020; Zou et al. 2022) on z-scores, independently for every LD block of the plan (blocks as
 * viprs_plan_get_blocks lists them, SNP order): z ~ N(R b, R) with the residual variance fixed at 1 (`susie_rss` with
 * estimate_residual_variance = FALSE), b = sum_{l < L} b_l, every b_l a single effect: exactly one SNP j is non-zero, chosen
 * with prior pi_j, its value N(0, V_l).  R = unit diagonal + dq_scale * stored off-diagonal entries: exactly the matrix of
 * viprs_plan_dot(..., include_diagonal = 1).  The reference tree has no fine-mapping model, so nothing here is a parity
 * claim: the definition below is the contract.
 *   z            (m,) doubles, finite
 *   log_prior    (m,) doubles, log pi_j; -inf excludes a SNP (not every SNP of a block); NULL: -log(block size), the host
 *                libm's log of the size as a double
 *   prior var.   V start: (n_blocks, L) row-major doubles, or NULL and `prior_variance0` for every effect; finite, >= 0
 *   state        alpha, mu, Rb: (m, L) column-major in the state precision T (`float_dtype`), all zero at the start;
 *                bbar, Y: (m,) in T; V, post_var: (n_blocks, L) doubles
 *   a step       effect l of iteration it (it = 1, 2, ...; l = 0 .. L - 1), for every SNP j of a block that is still running.
 *                Every operation below is one IEEE double operation on the values named, no contraction; (T)x is one rounding
 *                to the state precision, (double)x the exact conversion of a stored T value:
 *                  0. unless this is the first step of the call: Rb[j, (l - 1) mod L] = Y[j], the product launched by the
 *                     step before
 *                  1. a_j = ((0 + (double)Rb[j, l'_1]) + (double)Rb[j, l'_2]) + ... over l' != l in ascending l';
 *                     r_j = z_j - a_j.  Recomputed at every step: no running total
 *                  2. s = V_l / (1 + V_l);  w_j = (0.5 * (r_j * r_j)) * s + log pi_j;  mu[j, l] = (T)(s * r_j).
 *                     (-0.5 log(1 + V_l) of the log Bayes factor is constant over the block and cancels below)
 *                  3. wmax = max_j w_j;  e_j = exp(w_j - wmax) with the host libm's exp (glibc 2.35, bit for bit);
 *                     m_j = (double)mu[j, l];  S = sum_j e_j;  Q = sum_j e_j * (s + m_j * m_j)
 *                  4. alpha[j, l] = (T)(e_j / S);  bbar_j = (T)((double)alpha[j, l] * m_j);  post_var[l] = s
 *                  5. estimate_prior_variance: V_l <- Q / S (the EM update; it takes effect at the effect's next visit).
 *                     V_l = 0 needs no special case: alpha = pi, mu = 0
 *                  6. delta_it = max(delta_it, max_j |(double)alpha[j, l] - (double)alpha_old[j, l]|), alpha_old = what the
 *                     buffer held (0 before the first iteration); delta_it starts from 0 at l = 0
 *                  7. Y = R bbar is launched (viprs_plan_dot's kernels, one column, in T)
 *   order        S and Q are summed in the order of the ridge solve's dot products: 16-byte chunks of T (4 float32, 2
 *                float64 elements) dealt to 256 threads in turn, one double accumulator per thread adding in ascending
 *                order, the xor butterfly over the 64 lanes, the wavefronts in order.  The maxima are order-free.  No
 *                floating-point atomics
 *   stopping     after effect L - 1 of iteration it a block is converged (status 0) if delta_it < tol, otherwise stopped at
 *                max_iter (status 1) if it >= max_iter.  A block whose status is final is frozen: later launches leave every
 *                one of its outputs unchanged.  The number of running blocks is read back every `check_every` iterations:
 *                the only synchronisation inside the loop
 *   outputs      alpha, mu ((m, L) column-major, T), prior_variance_out (V after its last update), post_var_out, and per
 *                block iterations done, the last delta_it and the status (each of the last five may be NULL)
 * A block's bits depend on its own entries, its z, its log pi, L, the V start, tol, max_iter and its size: not on its place
 * in the plan, on the other blocks, on `check_every` or on timing; two calls give identical bits.
 * NOT BUILT: susieR's `optim` estimator of V and its null check, residual-variance estimation, the n-adjusted z of
 * susie_rss, lambda regularisation, several ranks, a fast-math variant, skipping the LD rows of frozen blocks (the product
 * streams the whole plan).  viprs_plan_set_active_blocks does NOT filter the call.  The workspace lives on the plan and is
 * reused.  Windowed plans and the dense blocks of the upper form are read as the product reads them.
 * Bad dtype code, L outside 1..32, tol <= 0, max_iter < 1, check_every < 1, dq_scale not finite or <= 0, a negative or
 * non-finite prior variance, a non-finite z, a log_prior that is NaN, +inf or -inf over a whole block, a null plan / z /
 * alpha / mu: VIPRS_EINVAL before any launch, outputs untouched.  An empty plan returns VIPRS_OK.
 *   viprs_plan_last_susie_ms  HIP-event time from the first to the last kernel of the last call on this plan (the read-backs
 *                             of the loop included), the step kernels it launched, and (nullable) the time of ONE step
 *                             kernel: effect L - 1 of iteration 1, when every block is still running */
int viprs_plan_susie(viprs_plan* plan, int float_dtype, int L, const double* z_host,
                     const double* log_prior_host /* nullable: -log(block size) */,
                     const double* prior_variance_host /* (n_blocks, L), or NULL with prior_variance0 */,
                     double prior_variance0, int estimate_prior_variance, double dq_scale,
                     double tol, int max_iter, int check_every,
                     void* alpha_host, void* mu_host,              /* (m, L) column-major, T */
                     double* prior_variance_out, double* post_var_out,   /* (n_blocks, L) */
                     int32_t* block_iters, double* block_delta, int32_t* block_status /* each nullable */);
int viprs_plan_last_susie_ms(viprs_plan* plan, double* total_ms, int* steps, double* step_kernel_ms);

/* ---- genotype scoring: PLINK .bed rows on the device, per-SNP code counts, polygenic scores ------------------------------
 * What a fitted model is for: score(i, c) = sum_j B[j, c] * dose_j(genotype of sample i at SNP j).  The reference hands this to
 * plink2 through magenpy (BayesPRSModel.predict -> GWADataLoader.predict); neither is part of the reference tree, so nothing
 * here claims parity with them: the definition below is this library's own, stated in full.
 * INPUT.  The rows of a PLINK 1 .bed file in SNP-major mode, WITHOUT the three magic bytes 6C 1B 01 (the reader checks and
 * strips them): m rows of ceil(n / 4) bytes.  Sample i of SNP j is bits 2 (i % 4) .. 2 (i % 4) + 1 of byte i / 4 of row j.
 * Codes: 0 = two copies of A1, 1 = missing, 2 = one copy, 3 = no copy.  The unused bits of a row's last byte are arbitrary;
 * no result depends on them.  1 <= n < 2^31 - 16 or n = 0; offsets into the rows are 64-bit everywhere.
 *   viprs_genotypes_create       device memory for m rows at a row stride that is a multiple of 16 bytes; every row starts
 *                                as "all samples missing" until it is uploaded
 *   viprs_genotypes_upload_rows  rows [first_row, first_row + n_rows) from `bed_rows` (n_rows x ceil(n / 4) bytes, as in the
 *                                file: a memory-mapped file goes up in slices).  The library then sets every slot at or beyond
 *                                n of those rows -- the file's own trailing bits and the stride padding -- to code 1
 *   viprs_genotypes_counts       counts[j][code] = the number of samples i < n with that code, int64, exact, all four codes
 * SCORE.  `b_host` is (m, n_cols) row-major in T = float32 / float64 (`float_dtype`), `dose_host` the per-SNP dose table
 * (m, 4) in T indexed by code; dose_host == NULL means {2, 0, 1, 0} for every SNP.  `scores_host` is (n, n_cols) row-major.
 *   term(i, j, c) = fl_T(B[j][c] * D[j][code(i, j)])                 one rounded multiply, no fma
 *   P(i, c, k)    = ((0 + term(i, j_k, c)) + term(i, j_k + 1, c)) + ...  plain T additions, SNPs ascending, over chunk
 *                                                                    k = SNPs [k L, min((k + 1) L, m)), L = VIPRS_SCORE_CHUNK
 *   score(i, c)   = fl_T(sum_k (double) P(i, c, k))                  double additions from 0, chunks ascending
 * L is part of the definition.  No floating-point atomics.  A column's bits depend on the genotypes, D and that column only:
 * not on n_cols, on the other columns, on padding or on how the work was tiled; two calls give identical bits.  Inputs are
 * finite; behaviour on NaN / inf is unspecified.  (An accumulator that starts at +0 never becomes -0 under these operations,
 * so leaving out a SNP whose B row is all zeros would be bit-identical; this library does not skip.)
 * DOSE TABLES are the caller's: additive with missing = 0 is {2, 0, 1, 0}; mean-imputed {2, mu_j, 1, 0} with
 * mu_j = (2 c0 + c2) / (c0 + c2 + c3) (0 when every sample is missing); standardised {(2 - mu) / s, 0, (1 - mu) / s, -mu / s}
 * with s_j the population standard deviation of the non-missing doses (a monomorphic SNP: all zeros); alleles swapped
 * relative to the model: entries 0 and 3 exchanged, mu' = 2 - mu.  Built on the host in double from the exact counts and
 * rounded once to T (viprs_amd/genotypes.py); the kernel knows only D.
 * ROUNDING.  |score - exact| <= (L + 2) u_T S + n_chunks 2^-53 S to first order, S = sum_j |B[j][c] D[j][code]|, u_T the unit
 * roundoff of T: L sequential additions of once-rounded terms, the double sum over the chunks, the final rounding.
 * Synchronous, on the object's own stream.  The partial sums P of a range of chunks go to a work buffer of bounded size
 * (at least one chunk: n x n_cols values, at most ~64 MiB otherwise; VIPRS_SCORE_WORK_BYTES in the environment sets another
 * budget) and a second kernel adds each range to the double sums; the result does not depend on the budget.
 * Bad dtype code, n_cols < 1, null pointers, rows out of range, n or m < 0: VIPRS_EINVAL before any launch, outputs untouched.
 * n = 0 or m = 0 is legal: counts and scores are zeros (n = 0: nothing to write).
 *   viprs_genotypes_last_score_ms   HIP-event time from the first to the last kernel of the last score call on this object
 *   viprs_genotypes_last_counts_ms  HIP-event time of the counts kernel of the last counts call (its download not included) */
#define VIPRS_SCORE_CHUNK 1024
typedef struct viprs_genotypes viprs_genotypes;
int viprs_genotypes_create(viprs_genotypes** g, int64_t n_samples, int64_t m, int device);
int viprs_genotypes_upload_rows(viprs_genotypes* g, int64_t first_row, int64_t n_rows, const uint8_t* bed_rows);
int viprs_genotypes_destroy(viprs_genotypes* g);
int viprs_genotypes_counts(viprs_genotypes* g, int64_t* counts /* m x 4 */);
int viprs_genotypes_score(viprs_genotypes* g, int float_dtype, int n_cols, const void* b_host,
                          const void* dose_host /* m x 4 in T, nullable */, void* scores_host /* n x n_cols */);
int viprs_genotypes_last_score_ms(viprs_genotypes* g, double* ms);
int viprs_genotypes_last_counts_ms(viprs_genotypes* g, double* ms);

/* ---- LD from genotypes: the correlation of the mean-imputed doses on the int8 matrix cores, in the compact upper store ----
 * magenpy and plink compute LD for the reference; neither is part of the reference tree, so nothing here claims parity with
 * them.  The definition below is the contract.
 * For SNP j and sample s < n the .bed code gives a dose x_sj and a presence p_sj:
 *   code 0: x = 2, p = 1;   code 2: x = 1, p = 1;   code 3: x = 0, p = 1;   code 1 (missing): x = 0, p = 0
 * Per SNP, from the exact counts c0..c3:
 *   nn_j = c0 + c2 + c3;  a_j = 2 c0 + c2;  q_j = 4 c0 + c2;  d_j = nn_j q_j - a_j^2 (int64)
 *   w_j = sqrt((double)(nn_j d_j)), computed ON THE HOST in double and handed in (`w`): as for the dose tables, what is built
 *   from the exact counts is built on the host
 * Per pair, four exact integer sums over the samples:
 *   S_ij = sum_s x_si x_sj;  U_ij = sum_s x_si p_sj;  U_ji = sum_s p_si x_sj;  N_ij = sum_s p_si p_sj
 *   num_ij = nn_i nn_j S_ij - nn_i a_j U_ij - nn_j a_i U_ji + a_i a_j N_ij      (int64, exact)
 *   r_ij   = (w_i == 0 || w_j == 0) ? 0.0 : (double)num_ij / (w_i * w_j)        (IEEE double, one rounding per operation, no fma)
 * This is the Pearson correlation of the mean-imputed doses: unit diagonal, positive semi-definite over the full sample;
 * a monomorphic or all-missing SNP gives 0.  The sums are integers accumulated exactly in int32 (v_mfma_i32_32x32x32_i8), so
 * the order of summation is not part of the definition: the result equals a NumPy int64 evaluation with ==.
 * OUTPUT element (`out_dtype`, ties to even as np.rint):
 *   VIPRS_LD_F64: r;   VIPRS_LD_F32: (float)r;   VIPRS_LD_I8: rint(r 127) clamped to +-127;   VIPRS_LD_I16: rint(r 32767)
 *   clamped to +-32767.  These are the stores' quantisation; dq_scale = 1 / max.
 * n <= 2^19 keeps every term and the sum inside int64 (4 n^3 4 < 2^63); a larger n: VIPRS_EINVAL before any device work.
 * WINDOWS.  right_end[j], j + 1 <= right_end[j] <= m, non-decreasing.  Row j of the store holds r_{j,k} for
 * k = j + 1 .. right_end[j] - 1: indptr[j + 1] - indptr[j] = right_end[j] - j - 1, no diagonal.
 * `data_host` receives rows [row0, row1) of the store, element indptr[row0] first; nothing else is written.  The caller
 * slices the rows so that the device buffer and the download stay bounded.  Synchronous, on the object's own stream.
 * NULL pointer, right_end not monotone or out of range, unknown dtype code, n > 2^19, row0 > row1 or rows outside [0, m]:
 * VIPRS_EINVAL before any device work, outputs untouched.
 *   viprs_genotypes_last_ld_ms   HIP-event time of the kernels of the last LD call on this object that launched any */
int viprs_genotypes_ld(viprs_genotypes* g, int64_t row0, int64_t row1, const int64_t* right_end /* m */,
                       const double* w /* m */, int out_dtype, void* data_host /* rows [row0,row1) of the store */);
int viprs_genotypes_last_ld_ms(viprs_genotypes* g, double* ms);

/* ---- per-genotype-class column sums: what an association test (GWAS) of the .bed rows is derived from ---------------------
 * One generic device operation; every association statistic is derived from it on the host in double
 * (viprs_amd/genotypes.py, `association`).  magenpy and plink2 compute the reference's GWAS; neither is part of the reference
 * tree, so nothing here claims parity with them.  The definition below is the contract.
 * `y_host` is (n, n_cols) row-major double, `sums_host` is (row1 - row0, 3, n_cols) row-major double.
 * CLASSES.  k = 0: code 0 (two copies of A1);  k = 1: code 2 (one copy);  k = 2: code 3 (no copy).  Code 1 (missing) belongs
 * to no class.  For SNP j, class k and column c:
 *   t(i)  = (class(i, j) == k) ? Y[i][c] : +0.0                       for the samples i < n
 *   s(i)  = (i >> 4) & 63                                             the slot of a sample, VIPRS_CLASS_SUM_SLOTS = 64 slots:
 *                                                                     the 16 samples of one 32-bit word of the row share a
 *                                                                     slot, and so do the words w, w + 64, w + 128, ...
 *   P[s]  = ((+0 + t(i1)) + t(i2)) + ...                              over the samples of slot s in ascending i: plain double
 *                                                                     additions (__dadd_rn), no fma, nothing reassociated
 *   butterfly: for d in 32, 16, 8, 4, 2, 1: P[s] <- P[s] + P[s ^ d]   all slots at once
 * IEEE addition is commutative, so after the last step all 64 values are identical: that value is sums[j - row0][k][c].
 * The bits of an output depend on row j's genotypes, column c and n only: not on n_cols, on the other columns, on row0 / row1,
 * on m, on any work-buffer budget or on how the work was tiled; two calls give identical bits.  An accumulator that starts at
 * +0 never becomes -0 under these additions, so adding +0.0 for a sample of another class is bit-identical to skipping it:
 * either implementation is allowed.  Y is finite; behaviour on NaN / inf is unspecified.  Slots at or beyond n read as code 1
 * (viprs_genotypes_upload_rows) and contribute nothing; a row that was never uploaded gives zeros.  n = 0 (zeros) and
 * row0 == row1 (nothing is written) are legal.
 * ROUNDING, to first order: |sum - exact| <= (16 ceil(n / 1024) + 6) 2^-53 sum|t|: the longest slot chain -- 16 samples per
 * word, ceil(n / 1024) words per slot -- plus the six butterfly steps.  Derived, not measured.
 * n_cols < 1, row0 > row1, a null pointer, rows outside [0, m]: VIPRS_EINVAL before the object is touched or anything is
 * launched, outputs untouched.  Synchronous, on the object's own stream; the stream is drained before the call's host buffers
 * go out of scope, on error paths too.  The caller slices the rows so that the output stays bounded.
 *   viprs_genotypes_last_class_sums_ms   HIP-event time of the kernels of the last class-sums call that launched any */
#define VIPRS_CLASS_SUM_SLOTS 64
int viprs_genotypes_class_sums(viprs_genotypes* g, int64_t row0, int64_t row1, int n_cols,
                               const double* y_host /* n x n_cols, row-major */,
                               double* sums_host /* (row1-row0) x 3 x n_cols, row-major */);
int viprs_genotypes_last_class_sums_ms(viprs_genotypes* g, double* ms);

/* ---- measurement support: synthetic LD generated on the device (bench.py, tests) --------------
 * The "longrange" LD blocks of viprs_amd/utils/synthetic.py (the workload of BASELINE.json's configs, SURVEY.md 8d: the
 * reference gets its LD from magenpy stores, VIPRS.py:151-172, none of which exists here) written straight into a plan's
 * device memory: a rank of a multi-GPU run has its genome-scale workload in milliseconds instead of generating 3.8 GB on
 * the host and uploading it.  `sizes`: n_blocks block sizes; pw / uf0 / uf1 / sa / sf: per-SNP float32 parameter
 * vectors (m = sum of sizes entries each; synthetic.longrange_device_params): entry (i, j) of a block is
 *   (uf0[i] uf0[j] + uf1[i] uf1[j]) + (pw[|i - j|] sa[i]) sf[j]  off the diagonal, 1 on it,
 * every operation rounded to float32; int8 / int16 LD stores rint(127 x) / rint(32767 x).  Layout, validation, block
 * discovery and re-lay-out are those of viprs_plan_create.  viprs_synthetic_ld_host runs the SAME function on the host
 * into the caller's row-concatenated array of `capacity` elements (the CPU test of the generator). */
int viprs_plan_create_synthetic(viprs_plan** plan, int64_t n_blocks, const int64_t* sizes, const float* pw,
                                const float* uf0, const float* uf1, const float* sa, const float* sf, int ld_dtype,
                                int low_memory, int device);
int viprs_synthetic_ld_host(int64_t n_blocks, const int64_t* sizes, const float* pw, const float* uf0, const float* uf1,
                            const float* sa, const float* sf, int ld_dtype, int low_memory, void* out, int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* VIPRS_HIP_H */
