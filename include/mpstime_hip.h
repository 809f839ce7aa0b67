/*
 * mpstime_hip.h - C ABI of libmpstime_hip.so, the MI355X (gfx950) sweep engine
 * for MPSTime.jl's DMRG-style training sweep.
 *
 * The reference (hugopstackhouse/MPSTime.jl) has no FFI: the seam this library
 * replaces is the Julia method
 *     fitMPS(W::MPS, training_states_meta, testing_states_meta, opts)
 *     src/Training/RealRealHighDimension.jl:587-890
 * selected at :556-560 / :578-582 (where `use_legacy_ITensor` already switches
 * engines).  Each entry point below cites the reference lines it stands in for.
 * INTEGRATION.md shows the Julia `ccall` shim that binds them.
 *
 * Conventions
 *   - plain C, no C++ types or exceptions cross the boundary;
 *   - every call returns 0 (MPST_OK) or a negative mpst_status; the message of
 *     the last failure on a context is available from mpst_last_error();
 *   - sites, classes and samples are 0-based here (the Julia shim converts);
 *   - the caller owns every host buffer, which only has to stay valid for the
 *     duration of the call; the library owns all device memory;
 *   - one caller thread per context; calls block until the device work is done
 *     unless stated otherwise.
 *
 * Data layouts at the boundary
 *   - encoded series  phi[N][T][d]   (d fastest, i.e. a Julia Array of size (d,T,N));
 *     series sorted by class (asserted, RealRealHighDimension.jl:621-625);
 *   - label_idx[N]    0-based class slot, non-decreasing;
 *   - site tensor j   column-major array of size (d, chi[j], chi[j+1]) and, on the
 *     label site, (d, chi[j], chi[j+1], C): element (s,l,r,c) at
 *     s + d*(l + chi[j]*(r + chi[j+1]*c)).  chi[0] = chi[T] = 1.
 *
 * Element types (opts.dtype, RealRealHighDimension.jl:442).  A context has ONE element type - MPST_F64 (default), MPST_F32,
 *   MPST_C128, MPST_C64 - fixed by its first data set (mpst_set_dataset's `dtype`, or mpst_set_dtype before a device-side
 *   encoding): encoded series and site tensors cross the boundary in that type (complex: interleaved (re, im), i.e. Julia's
 *   ComplexF64 / ComplexF32 arrays).  Complex encodings (Fourier, Sahand, Stoudenmire) need a complex type, as in the reference
 *   (RealRealHighDimension.jl:461-466); their training follows the reference's legacy ITensor engine, the only one that
 *   accepts them (src/legacy_itensor/loss_functions.jl:433-640, RealRealLegacyITensor.jl:2-142): phi~ = conj(ps_l) (x) LE (x)
 *   conj(ps_r) (x) RE, yhat = BT * phi~ (no conjugate on BT), loss -log|yhat|^2, grad = -conj(phi~ / yhat).  Whatever the
 *   element type, overlaps, losses, the reduced gradient, the optimiser step, the Gram matrix of the bond tensor and its
 *   eigen-decomposition are fp64; scalar results (losses, spectra, overlaps) are returned as doubles ((re, im) pairs of
 *   doubles for the overlaps of a complex context).
 */
#ifndef MPSTIME_HIP_H
#define MPSTIME_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: mpst_get_info writes 16 entries (1: 12), mpst_set_dtype / mpst_get_info_n added, element types other than Float64
 *    accepted by mpst_set_dataset / mpst_set_mps.  A host compares mpst_version() with the header it was built against.
 *    The number moves when a declared function or struct changes its layout or meaning; functions added beside the existing
 *    ones (mpst_impute_traj, mpst_impute_model_traj, mpst_impute_dist, mpst_impute_model_dist, mpst_marginal_model, mpst_site_conditionals, mpst_pair_analysis, mpst_window_conditionals, mpst_marginal_conditionals, mpst_observed_conditionals) and entries appended to a getter that takes its length
 *    (mpst_get_impute_info) leave every existing caller valid and do not move it. */
#define MPST_ABI_VERSION 2

typedef enum {
    MPST_OK = 0,
    MPST_ERR_INVALID = -1,      /* bad argument / call order (Julia: ArgumentError) */
    MPST_ERR_UNSUPPORTED = -2,  /* option combination the engine lacks (Julia: ErrorException, cf. loss_functions.jl:166-170) */
    MPST_ERR_DEVICE = -3,       /* HIP / RCCL runtime failure */
    MPST_ERR_SVD = -4,          /* bond-tensor decomposition failed / non-finite spectrum; the
                                   class of failure tune() retries on (hyperparameters/tuning.jl:73-86) */
    MPST_ERR_NOMEM = -5
} mpst_status;
enum { MPST_ERR_DOMAIN = -6 };   /* rho_correct: RDM eigenvalue < -sqrt(eps) or trace off by > 0.01 (Julia: DomainError) */

enum { MPST_LOSS_KLD = 0, MPST_LOSS_MSE = 1 };   /* src/Structs/options.jl:318-327 */
enum { MPST_OPT_TSGO = 0, MPST_OPT_GD = 1 };     /* src/Structs/options.jl:298-311 */
enum { MPST_F64 = 0, MPST_F32 = 1, MPST_C128 = 2, MPST_C64 = 3 };
enum { MPST_SVD_DEFAULT = 0, MPST_SVD_JACOBI = 1 };  /* opts.svd_alg, RealRealHighDimension.jl:756,798 */
enum { MPST_TRAIN = 0, MPST_TEST = 1 };

/* The MPSOptions fields the sweep consumes
 * (src/Structs/options.jl:106-143; RealRealHighDimension.jl:591-592,606,716-722). */
typedef struct {
    int32_t chi_max;            /* opts.chi_max  (:720) */
    int32_t update_iters;       /* opts.update_iters (:716) */
    int32_t loss;               /* MPST_LOSS_*  <- opts.loss_grad */
    int32_t optimiser;          /* MPST_OPT_*   <- opts.bbopt */
    int32_t rescale_before;     /* opts.rescale[1]  (loss_functions.jl:109) */
    int32_t rescale_after;      /* opts.rescale[2]  (loss_functions.jl:177) */
    int32_t train_classes_separately;  /* TrainSeparate{B} (:606) */
    int32_t svd_alg;            /* MPST_SVD_* */
    int32_t rebuild_caches;     /* 1: redo both full cache rebuilds per sweep as the reference does
                                   (:770,:804); 0: skip them (bit-identical results) */
    int32_t track_cost;         /* opts.track_cost (loss_functions.jl:50-52,80-82,181-184): record the loss before every
                                   optimiser step and at the updated bond tensor; read them with mpst_get_loss_trace */
    double  eta;                /* opts.eta (:719) */
    double  cutoff;             /* opts.cutoff (:722) */
} mpst_options;

/* Per-sweep result of mpst_sweep (RealRealHighDimension.jl:727,806-808). */
typedef struct {
    double  seconds;            /* device time of the sweep (HIP events) */
    int32_t svd_status;         /* 0 or MPST_ERR_SVD */
    int32_t max_chi;            /* largest bond dimension after the sweep */
    int32_t eig_sweeps_total;   /* diagnostic: Jacobi sweeps summed over the bonds of this sweep */
    int32_t eig_fallbacks;      /* diagnostic: bonds of this sweep on which the fast eigensolver's on-device
                                   verification failed and the Jacobi path was used */
} mpst_sweep_stats;

/* Test hook output of mpst_bond_step: gauge-invariant per-bond quantities. */
#define MPST_MAX_SPECTRUM 512
typedef struct {
    double  loss;               /* loss before the (first) step, loss_functions.jl:371 */
    double  grad_norm;          /* ||grad||_F of the first iteration (:79) */
    double  bt_norm;            /* ||bt_new||_F before the rescale (:177) */
    int32_t chi_new;            /* kept bond dimension after truncation */
    int32_t n_spectrum;         /* number of entries valid in spectrum[] */
    int32_t eig_sweeps;
    int32_t reserved;
    double  spectrum[MPST_MAX_SPECTRUM];  /* all singular values of the (rescaled) bond tensor, descending */
} mpst_bond_debug;

int         mpst_version(void);
const char* mpst_last_error(void* ctx);           /* never freed by the caller; NULL ctx -> creation errors */

/* One context per GPU (one process per GPU).  Replaces nothing in the reference:
 * device selection is new. */
int  mpst_create(void** ctx, int device_id);
void mpst_destroy(void* ctx);

/* Batch sharding over GPUs (new design): every rank holds N/G series;
 * the bond gradient + loss are all-reduced with RCCL once per optimiser step.
 * `unique_id` is the 128-byte ncclUniqueId produced on rank 0 and distributed by the host. */
int  mpst_comm_unique_id(uint8_t out_id[128]);
int  mpst_comm_init(void* ctx, const uint8_t unique_id[128], int nranks, int rank);
/* librccl is bound at run time, not linked: MPST_RCCL_LIB if set, else the copy the host process has already loaded (a
 * Python host that imported torch holds torch's own librccl.so.1), else /opt/rocm/lib's - never two copies in one process.
 * Reports "<path> (<how it was found>)" (or the reason it could not be loaded), the library's ncclGetVersion code and the
 * NCCL_VERSION_CODE of the header this library was compiled against; mpst_comm_init refuses another major version. */
int  mpst_comm_library(char* path_out, int32_t path_cap, int32_t* version_out, int32_t* built_against_out);

/* One-shot direct-write all-reduce over xGMI, next to the RCCL path (the 262 KB message is latency-bound).
 * Every rank allocates an inbox in fine-grained device memory and exports it (64-byte hipIpcMemHandle_t); the host
 * gathers the handles of all ranks (torch.distributed all_gather, MPI, ...) and hands the rank-ordered array to
 * mpst_comm_ipc_attach, after which gradient and evaluation sums go through the one-shot kernel (peer writes + flags,
 * fixed rank-order sum: bit-identical replicas).  Call after mpst_set_options / mpst_set_dataset / mpst_set_mps (the slot
 * size follows the gradient buffer) and again if those change the capacity.  RCCL is not required: without
 * mpst_comm_init the pair (export, attach) alone defines the communicator.  mpst_comm_select switches between the two
 * paths when both exist (0 = RCCL, 1 = one-shot).  2..8 ranks (one node). */
int  mpst_comm_ipc_export(void* ctx, int nranks, int rank, uint8_t handle_out[64]);
int  mpst_comm_ipc_attach(void* ctx, const uint8_t* all_handles /* nranks * 64 bytes, rank order */);
int  mpst_comm_select(void* ctx, int oneshot);

/* EncodedTimeSeriesSet -> device (src/Structs/structs.jl:12-33).  `n_global_per_class`
 * may be NULL on a single GPU; with sharding it carries the global class counts that
 * the loss normalisation uses (loss_functions.jl:367,371,423-424).
 * A rejected call of this function or of mpst_encode_[split_]dataset leaves the context
 * exactly as it was, the old set included; one that fails later (allocation, copy, sigmoid
 * fit) leaves set `which` empty (N = 0). */
int  mpst_set_dataset(void* ctx, int which, const void* phi, const int32_t* label_idx,
                      int64_t N, int32_t T, int32_t d, int32_t C, int32_t dtype,
                      const int64_t* n_global_per_class);
/* opts.dtype ahead of a device-side encoding (mpst_encode_dataset encodes in fp64 and stores in this type; without it a
 * real basis gives MPST_F64 and a complex basis MPST_C128).  Must precede the data sets and the MPS. */
int  mpst_set_dtype(void* ctx, int32_t dtype);

/* Device-side preprocessing + encoding: the raw N x T matrix (row-major, already sorted by
 * class like mpst_set_dataset's input) goes through transform_train_data / transform_test_data
 * (src/utils.jl:161-275) and the Legendre basis (src/Encodings/bases.jl:70-108) on the GPU and becomes data set
 * `which`, instead of uploading the d times larger product states (encode_dataset,
 * src/Encodings/encodings.jl:120-150).  `median`, `iqr` are the
 * RobustSigmoid parameters of the TRAINING set (Normalization.jl fit, utils.jl:171-176) - inputs, or, with
 * fit_sigmoid = 1 on a training set, OUTPUTS fitted on the device (radix sort of the N T values, type-7
 * quantiles).  Training set
 * (is_test = 0): the min / max of the sigmoid-transformed data are fitted on the device and returned in
 * lo / hi.  Test set (is_test = 1): lo / hi are inputs (the training fit); with rescale_out_of_bounds each
 * series is shifted / scaled into [0, 1] (utils.jl:243-266) and `oob_fix` ([N][2], may be NULL) receives the
 * (shift, scale) applied to every series - (0, 1) where nothing was done.  `seconds` (may be NULL) receives
 * the device time of the encoding kernels. */
#define MPST_BASIS_LEGENDRE         0   /* legendre(norm = true),  bases.jl:81-92 */
#define MPST_BASIS_LEGENDRE_NO_NORM 1   /* legendre_no_norm,       bases.jl:108  (MPSOptions default) */
#define MPST_BASIS_FOURIER          2   /* fourier_encode,         bases.jl:23-42 (mpst_encode_values; mean method of complex models) */
/* the remaining closed-form bases: */
#define MPST_BASIS_STOUDENMIRE      3   /* angle_encode, d = 2,    bases.jl:7-21  (complex) */
#define MPST_BASIS_SAHAND           4   /* sahand_encode, even d,  bases.jl:45-68 (complex) */
#define MPST_BASIS_UNIFORM          5   /* uniform_encode,         bases.jl:2-4   (real) */
typedef struct {
    int32_t basis;
    int32_t sigmoid_transform;      /* MPSOptions.sigmoid_transform */
    int32_t minmax;                 /* MPSOptions.minmax */
    int32_t is_test;
    int32_t rescale_out_of_bounds;  /* test sets only */
    int32_t fit_sigmoid;            /* training sets only: fit median / iqr on the device */
    double  median, iqr;            /* in, or out with fit_sigmoid */
    double  lo, hi;                 /* out for the training set, in for a test set */
    double  data_lb, data_ub;       /* MPSOptions.data_bounds */
    double  range_a, range_b;       /* the basis' input range (-1, 1 for Legendre) */
} mpst_encode_opts;
int  mpst_encode_dataset(void* ctx, int which, const double* X, const int32_t* label_idx,
                         int64_t N, int32_t T, int32_t d, int32_t C, mpst_encode_opts* eo,
                         const int64_t* n_global_per_class, double* oob_fix, double* seconds);
/* The same preprocessing + encoding kernels without a data set: X[N][T] in, the encoded states out to the host,
 * phi_out[N][T][d] doubles for the Legendre bases or (re, im) pairs for MPST_BASIS_FOURIER (fourier_encode,
 * bases.jl:23-42: cispi(f x) / sqrt(d), f = 0, 1, -1, 2, -2, ...) - what mpst_impute_model_run takes for a complex model.
 * eo as for mpst_encode_dataset (fits returned in it); oob_fix [N][2] or NULL. */
int  mpst_encode_values(void* ctx, const double* X, int64_t N, int32_t T, int32_t d, mpst_encode_opts* eo, void* phi_out,
                        double* oob_fix, double* seconds);
/* Split bases (src/Encodings/splitbases.jl; histogram_split / uniform_split, basis_structs.jl:247-279): the input range is cut
 * into nbins bins, every bin carries its own copy of an auxiliary closed-form basis of aux_dim states, d = nbins * aux_dim.  A value
 * in bin i is encoded as the auxiliary basis at a + (b - a) (x - bins[i]) / (bins[i+1] - bins[i]) in the entries of bin i and zero
 * elsewhere; a value exactly on an interior edge gives half of the auxiliary state in both neighbours, the outermost edges weight 1
 * (rect and project_onto_bins, splitbases.jl:96-132, same comparisons on the same expression; an empty bin selects nothing).
 *   aux_basis  MPST_BASIS_* of the auxiliary basis (Stoudenmire: aux_dim = 2, Sahand: even aux_dim)
 *   bins       the edges the host fitted (hist_split :56-92 per time point, unif_split :51-54), non-decreasing, in the encoding's
 *              range: [T][nbins + 1] with per_site = 1 (histogram_split), [nbins + 1] shared by all sites with per_site = 0
 * mpst_encode_split_dataset / mpst_encode_split_values are mpst_encode_dataset / mpst_encode_values with eo->basis ignored in favour
 * of sp->aux_basis.  MPST_ERR_INVALID: NULL sp / bins, nbins < 1 or > 512, d != nbins * aux_dim, decreasing edges;
 * MPST_ERR_UNSUPPORTED: an auxiliary basis outside the six, Stoudenmire with aux_dim != 2, Sahand with odd aux_dim. */
typedef struct {
    int32_t aux_basis, aux_dim, nbins, per_site;
    const double* bins;
} mpst_split_opts;
int  mpst_encode_split_dataset(void* ctx, int which, const double* X, const int32_t* label_idx,
                               int64_t N, int32_t T, int32_t d, int32_t C, mpst_encode_opts* eo, const mpst_split_opts* sp,
                               const int64_t* n_global_per_class, double* oob_fix, double* seconds);
int  mpst_encode_split_values(void* ctx, const double* X, int64_t N, int32_t T, int32_t d, mpst_encode_opts* eo,
                              const mpst_split_opts* sp, void* phi_out, double* oob_fix, double* seconds);
/* Sahand-Legendre bases (src/Encodings/bases.jl:111-129; sahand_legendre, basis_structs.jl:141-151): d polynomials orthonormalised
 * under the square root of a kernel density estimate of the training values, fitted on the host ("Sahand-Legendre
 * encodings").  A value x at site t is encoded as
 *   phi_n(x) = max(sqrt(max(pdf_t(x), 0)), minx_t) / scale_t * sum_i cvecs_t[n][i] x^i,      n = 0 .. d-1
 * where pdf_t is the quadratic B-spline through the estimate's npoints grid values: with u = (x - lo) / step + 1, i = round(u)
 * clamped to 1 .. npoints and s = u - i it is coef[i-1] (s - 1/2)^2 / 2 + coef[i] (3/4 - s^2) + coef[i+1] (s + 1/2)^2 / 2 inside
 * [lo, lo + (npoints - 1) step] and 0 outside.  A site whose cvecs are all zero encodes to zeros; its other tables are not read.
 * mpst_encode_kde_dataset / mpst_encode_kde_values are mpst_encode_dataset / mpst_encode_values with this basis: eo->basis is
 * ignored and not written (the states are real); the tables are copied to the device for the call and released with it.
 * MPST_ERR_INVALID: NULL kd or array, npoints < 3, per_site not 0 / 1, d < 1 or d > 16, and - at a site whose cvecs are not all
 * zero - a step, scale or minx that is not positive and finite. */
typedef struct {
    int32_t npoints, per_site;      /* K; 0: one table for all sites, 1: T tables */
    const double* lo;               /* [S], S = per_site ? T : 1 */
    const double* step;             /* [S] */
    const double* coef;             /* [S][K + 2] */
    const double* minx;             /* [S] */
    const double* scale;            /* [S] */
    const double* cvecs;            /* [S][d][d], row n = function n, column i = power i */
} mpst_kde_opts;
int  mpst_encode_kde_dataset(void* ctx, int which, const double* X, const int32_t* label_idx,
                             int64_t N, int32_t T, int32_t d, int32_t C, mpst_encode_opts* eo, const mpst_kde_opts* kd,
                             const int64_t* n_global_per_class, double* oob_fix, double* seconds);
int  mpst_encode_kde_values(void* ctx, const double* X, int64_t N, int32_t T, int32_t d, mpst_encode_opts* eo,
                            const mpst_kde_opts* kd, void* phi_out, double* oob_fix, double* seconds);
/* Projected bases (legendre(project = true), fourier(project = true): basis_structs.jl:114-139, bases.jl:94-107, :345-397): the
 * closed-form family, of which every site evaluates its own list of d members, chosen on the host ("Projected bases").
 * A value x at site t is encoded, slot j = 0 .. d-1, as
 *   MPST_BASIS_LEGENDRE_NO_NORM   sqrt((2k + 1) / 2) P_k(x),                k = orders[t][j]   (Bonnet recursion, as mpst_encode_values)
 *   MPST_BASIS_LEGENDRE           the same times inv_norm[t]
 *   MPST_BASIS_FOURIER            cispi(f x) / sqrt(d), an (re, im) pair,   f = orders[t][j]   (signed)
 * The list of a site need not be sorted and may repeat an order.  inv_norm is read for MPST_BASIS_LEGENDRE only and may be NULL
 * otherwise.  max_order bounds every |orders[t][j]|.
 * mpst_encode_proj_dataset / mpst_encode_proj_values are mpst_encode_dataset / mpst_encode_values with this basis: eo->basis is
 * ignored and not written; the tables are copied to the device for the call and released with it.
 * MPST_ERR_INVALID: NULL pj or orders; a basis other than the three above; d < 1 or d > 16; max_order < 0, above 7 * 16 (Legendre)
 * or above 5 * 16 (Fourier); an order below 0 (Legendre) or with |order| > max_order; MPST_BASIS_LEGENDRE with a NULL inv_norm or
 * an entry of it that is not positive and finite.  Every entry is checked before anything is launched. */
typedef struct {
    int32_t basis;                  /* MPST_BASIS_LEGENDRE / _LEGENDRE_NO_NORM / _FOURIER */
    const int32_t* orders;          /* [T][d]: Legendre orders, or signed Fourier frequencies */
    const double* inv_norm;         /* [T], or NULL */
    int32_t max_order;
} mpst_proj_opts;
int  mpst_encode_proj_dataset(void* ctx, int which, const double* X, const int32_t* label_idx,
                              int64_t N, int32_t T, int32_t d, int32_t C, mpst_encode_opts* eo, const mpst_proj_opts* pj,
                              const int64_t* n_global_per_class, double* oob_fix, double* seconds);
int  mpst_encode_proj_values(void* ctx, const double* X, int64_t N, int32_t T, int32_t d, mpst_encode_opts* eo,
                             const mpst_proj_opts* pj, void* phi_out, double* oob_fix, double* seconds);
/* Encoded values of data set `which` back to the host, [N][T][d] in the context's element type
 * (EncodedTimeSeriesSet.timeseries). */
int  mpst_get_encoded(void* ctx, int which, double* phi_out);

int  mpst_set_options(void* ctx, const mpst_options* o);

/* MPS in / out (the W::MPS argument and the TrainedMPS.mps result). `site[j]` points at
 * site tensor j in the boundary layout above; `label_site` is where the "f(x)" index
 * lives (utils.jl:342-354); training requires T-1 on entry (:19-29). */
int  mpst_set_mps(void* ctx, const void* const* site, const int32_t* chi, int32_t T, int32_t label_site);
int  mpst_get_chi(void* ctx, int32_t* chi_out /*[T+1]*/, int32_t* label_site);
int  mpst_get_mps(void* ctx, void* const* site_out /* T buffers sized from mpst_get_chi */);

/* construct_caches, RealRealHighDimension.jl:45-103,631: the left environments of every site left of
 * the label site and the right environments of every site right of it.  With the label on the last
 * site (the state training starts from) this is construct_caches(W, ...; going_left=true). */
int  mpst_build_caches(void* ctx);

/* One full sweep = RealRealHighDimension.jl:727-808. */
int  mpst_sweep(void* ctx, mpst_sweep_stats* out);

/* One sweep of K independent fits of the same shape in ONE launch chain: contexts with the same T, d, C, chi_max, capacity
 * and loss on one device; the number of series and the class counts may differ, as between the folds of a stratified k-fold split
 * (a fit whose series count moves its gradient share count is refused: batch it with its likes) (hyper-parameter candidates that share the shape - eta, cutoff, the data, the starting MPS
 * may differ -, CV folds, restarts; the reference runs such fits as separate @distributed tasks, hyperparameters/tuning.jl).
 * Every kernel launch carries all K fits, so a sweep costs the ~1200 launches of ONE fit: K separate contexts driven from K host
 * threads reach 2.3x a single fit on one MI355X (the dispatch rate is the limit), one batched chain about 5-6x for K = 8.
 * Results are those of K mpst_sweep calls, bit for bit.  Headline chain only (Float64, d*chi_max <= 128, <= 8192 series, one rank,
 * update_iters = 1, no track_cost / rebuild_caches / profiling): MPST_ERR_UNSUPPORTED otherwise - drive such fits one by one.
 * `out` ([K], may be NULL): seconds = device time of the whole batch.  Errors are reported on ctxs[0]. */
int  mpst_sweep_batch(void* const* ctxs, int32_t K, mpst_sweep_stats* out);
/* The same for fits dealt over SEVERAL devices of a node (what scales there: the batch-sharded sweep repeats its eigensolver on every
 * rank, independent fits share nothing): the contexts are grouped - group[k] is an arbitrary id, NULL = one group per device -, a
 * group must live on one device and hold fits of one shape (<= 64), and every group is advanced by ONE mpst_sweep_batch on its own
 * host thread, concurrently with the others.  No collective, no data crosses devices.  Results are those of K mpst_sweep calls, bit
 * for bit; out[k].seconds is the device time of fit k's group.  The reference's counterpart is the @distributed loop over candidate
 * fits (hyperparameters/hyperopt_utils.jl:201, tuning.jl). */
int  mpst_sweep_batch_multi(void* const* ctxs, int32_t K, const int32_t* group /* [K] or NULL */, mpst_sweep_stats* out);
/* Optional, before the first sweep of a context: it will be advanced in batches of about K fits.  The engine then splits every
 * gradient block of THIS fit into fewer shares (K fits fill the chip together); the share count fixes the order of the partial
 * sums, so mpst_sweep on the same context gives the same bits as mpst_sweep_batch, while a context without the hint differs from
 * it in the last bits of the gradient. */
int  mpst_set_batch_hint(void* ctx, int32_t K);

/* opts.track_cost: the losses the reference prints during the last mpst_sweep, one row per bond in sweep order (backward
 * half-sweep first): update_iters entries "Loss before step i" (loss_functions.jl:50-52 / :80-82) followed by the loss
 * at the updated bond tensor, "Loss at site lid*rid" (:181-184).  out has 2(T-1) * (update_iters + 1) entries. */
int  mpst_get_loss_trace(void* ctx, double* out);

/* One bond update (:733-762 going left, :777-801 going right) - test hook. */
int  mpst_bond_step(void* ctx, int32_t lid, int32_t going_left, mpst_bond_debug* dbg);

/* MSE_loss_acc / MSE_loss_acc_conf, src/summary.jl:33-114.  conf is C*C row-major
 * [truth][prediction] (may be NULL). */
int  mpst_eval(void* ctx, int which, double* mse, double* kld, double* acc, int64_t* conf);

/* classify(mps, states), src/summary.jl:116-136: predicted class slot per series,
 * and optionally the raw overlaps yhat[N][C] (complex context: [N][C][2], (re, im)). */
int  mpst_classify(void* ctx, int which, int32_t* pred /*[N]*/, double* yhat /*[N][C] or NULL*/);

/* The scoring step of tune / evaluate (hyperparameters/tuning.jl:1-207, hyperopt_utils.jl:152-231; classify and MSE_loss_acc of
 * src/summary.jl:4-136) for K models at once, each on its OWN data set `which`: one kernel launch walks every chain (a workgroup
 * keeps the environments of its 16 series on chip over all sites, the label site last), a second one forms the losses and the
 * confusion matrices - against T + 2 launches per model of mpst_eval / mpst_classify.  Float64 real contexts on one device and
 * one rank that share T, d and C, with d * capacity <= 128 (the batched chain's limit); the sets' sizes and the bond dimensions
 * may differ.  MPST_ERR_UNSUPPORTED otherwise - score such fits with mpst_classify.  The contexts' training caches are left
 * alone: a sweep after the call continues as if it had not happened.
 * pred[k] ([N_k] class slots), yhat[k] ([N_k][C] overlaps): NULL arrays or entries are skipped; loss3 ([K][3]: mean MSE, mean
 * KLD, accuracy) and conf ([K][C][C], [truth][prediction]) may be NULL.  Errors are reported on ctxs[0]. */
int  mpst_classify_batch(void* const* ctxs, int32_t K, int which, int32_t* const* pred, double* const* yhat, double* loss3, int64_t* conf);

/* Imputation of missing values, batched over the instances of data set `which`:
 * impute_median / impute_mode / impute_ITS of src/Imputation/MPS_methods.jl:198-330, i.e. precondition (:42-99) +
 * impute_at! (:103-177) with get_median_from_rdm / get_mode_from_rdm / get_sample_from_rdm (sampling_utils.jl:98-275),
 * for every instance at once instead of one @distributed task per instance.  The context holds the trained MPS (label
 * index anywhere); instance i is imputed with the class MPS of its label (expand_label_index, utils.jl:356-370).
 *   missing[N][T]   1 where the value is to be imputed (row-major, instances in the order of the data set);
 *                   the encoded values the data set holds at those sites are ignored
 *   grid_x[ngrid]   the candidate values x_k (range(guess_range...; step = dx), imputation.jl:90) and
 *   grid_phi[ngrid][d]  their encoded states (time-independent encodings, :100-106); with o->grid_per_site = 1
 *                   grid_phi[T][ngrid][d], one table per site (time-dependent encodings, :92-99): the state of grid value k at
 *                   site t is row t * ngrid + k.  A per-site table is never recognised as a closed-form grid: the call evaluates
 *                   the densities from the table, one instance per workgroup.  MPST_IMPUTE_MEAN with it: MPST_ERR_UNSUPPORTED
 *   o->method       MPST_IMPUTE_MEDIAN (+ weighted median absolute deviation when get_err), MPST_IMPUTE_MODE,
 *                   MPST_IMPUTE_QUANTILE: inverse-transform sampling with the caller's uniform numbers (impute_ITS with
 *                   rejection_threshold = :none; the reference draws them from a MersenneTwister),
 *                   MPST_IMPUTE_MEAN: expectation value (+ standard deviation when get_err), impute_mean :232-265 with
 *                   get_mean_from_rdm, sampling_utils.jl:66-96; the state the chain is re-conditioned on is the encoding
 *                   of the expectation value itself, evaluated on the device with the closed form of the basis (mean_basis:
 *                   MPST_BASIS_LEGENDRE / _LEGENDRE_NO_NORM / _UNIFORM for real models, _FOURIER / _STOUDENMIRE / _SAHAND
 *                   for complex ones; the data-driven bases have no closed form and are not supported),
 *                   MPST_IMPUTE_ITS_REJECT: get_sample_from_rdm with a rejection threshold (:271-296): median and WMAD
 *                   first, then up to max_trials inverse-transform samples, the first one within
 *                   rejection_threshold * WMAD of the median is kept (the last one drawn if none is); err_out = WMAD
 *   o->order        MPST_IMPUTE_FORWARDS / MPST_IMPUTE_BACKWARDS (impute_order, MPS_methods.jl:107-121): the missing
 *                   sites are visited left to right / right to left, each conditioned on the ones already imputed
 *   u[N][T][max_trials]  uniform numbers in [0, 1) for the two sampling methods (max_trials = 1 for QUANTILE), else NULL
 *   x_out[N][T]     imputed value at every missing site (in the encoding's domain; 0 elsewhere), err_out[N][T] the
 *                   uncertainty measure of the method (0 where there is none)
 * chi_max <= 128, d <= 16, real fp64. */
enum { MPST_IMPUTE_MEDIAN = 0, MPST_IMPUTE_MODE = 1, MPST_IMPUTE_QUANTILE = 2, MPST_IMPUTE_MEAN = 3, MPST_IMPUTE_ITS_REJECT = 4 };
enum { MPST_IMPUTE_FORWARDS = 0, MPST_IMPUTE_BACKWARDS = 1 };
typedef struct {
    int32_t method;
    int32_t order;
    int32_t get_err;                /* get_wmad (median) / get_std (mean) */
    int32_t max_trials;             /* ITS_REJECT only (reference default 10) */
    int32_t mean_basis;             /* MEAN only */
    int32_t grid_per_site;          /* 0: grid_phi[ngrid][d] shared by all sites, 1: grid_phi[T][ngrid][d]; else MPST_ERR_INVALID */
    double  rejection_threshold;    /* ITS_REJECT only */
} mpst_impute_opts;
int  mpst_impute(void* ctx, int which, const uint8_t* missing, const double* grid_x, const double* grid_phi, int32_t ngrid,
                 const mpst_impute_opts* o, const double* u, double* x_out, double* err_out, double* seconds);

/* The same engine on a model handed over in one call instead of through the context's data set and MPS - what an
 * imputation-only caller has (init_imputation_problem, imputation.jl:143-190, takes a trained MPS and test data) - and
 * the only door for the element types the sweep does not train:
 *   dtype    MPST_DTYPE_C64: site tensors, encoded values and grid states are complex (interleaved re, im doubles) - the
 *            reference's Fourier / Sahand bases (bases.jl:23-68), trained through its legacy ITensor path.  Known sites are
 *            projected with the conjugate state (dag(timeseries_enc), MPS_methods.jl:17), densities are |rho phi|^2.
 *   compute  MPST_COMPUTE_F32: the chain contractions (site tensors, environment matrices, boundary vectors) are stored
 *            and multiplied in fp32 (MFMA f32 16x16x4); the density on the grid, its cumulative sums and every selection
 *            stay fp64.  MPST_COMPUTE_F64: everything fp64.
 * site[j]: (s, l, r) column-major, the label site (s, l, r, c), like mpst_set_mps; phi: [N][T][d]; label_idx[N] in [0, C)
 * in any order.  chi_max <= 128, d <= 16.  mean_basis MPST_BASIS_FOURIER / _STOUDENMIRE / _SAHAND for complex models. */
#define MPST_DTYPE_F64   0
#define MPST_DTYPE_C64   1
#define MPST_COMPUTE_F64 0
#define MPST_COMPUTE_F32 1
typedef struct {
    int64_t N;
    int32_t T, d, C, label_site;
    int32_t dtype, compute;
    const void* const* site;
    const int32_t* chi;                 /* [T+1] */
    const void* phi;
    const int32_t* label_idx;
} mpst_impute_model;
int  mpst_impute_model_run(void* ctx, const mpst_impute_model* m, const uint8_t* missing, const double* grid_x, const void* grid_phi,
                           int32_t ngrid, const mpst_impute_opts* o, const double* u, double* x_out, double* err_out, double* seconds);

/* Several trajectories per instance (impute_ITS(...; num_trajectories), src/Imputation/MPS_methods.jl:304-347): the instance is
 * conditioned on its known values ONCE - the environment pass, one workgroup per instance exactly as in the calls above - and
 * K chains (instance, trajectory) are then sampled from that one conditioned MPS, the K chains of an instance next to each other.
 * mpst_impute_traj is mpst_impute, mpst_impute_model_traj is mpst_impute_model_run, with
 *   K               trajectories per instance; K < 1: MPST_ERR_INVALID.  K = 1 with u is the single-trajectory call, bit for bit.
 *   o->method       MPST_IMPUTE_QUANTILE or MPST_IMPUTE_ITS_REJECT; the other methods have one answer per instance:
 *                   MPST_ERR_UNSUPPORTED
 *   u[N][K][T][max_trials]  uniform numbers in [0, 1) (max_trials = 1 for QUANTILE), or NULL: they are then generated on the device
 *   seed, row_id[N] (u == NULL) Philox4x32-10 with the key (seed low word, seed high word) and the counter
 *                   (row id low word, row id high word, trajectory, site + trial * 2^20), sites and trajectories counted from 0;
 *                   the uniform number is ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53 of the output words w0, w1.  row_id names the
 *                   caller's rows (NULL: the index in the data set's order), so a draw depends neither on how the call was cut
 *                   into blocks, nor on which rows were sent along, nor on their order.  T <= 2^20, max_trials <= 4096.
 *   x_out[N][K][T], err_out[N][K][T]  as above, per chain; err_out is the chain's WMAD at every imputed site for ITS_REJECT */
int  mpst_impute_traj(void* ctx, int which, const uint8_t* missing, const double* grid_x, const double* grid_phi, int32_t ngrid,
                      const mpst_impute_opts* o, int32_t K, const double* u, int64_t seed, const int64_t* row_id, double* x_out,
                      double* err_out, double* seconds);
int  mpst_impute_model_traj(void* ctx, const mpst_impute_model* m, const uint8_t* missing, const double* grid_x, const void* grid_phi,
                            int32_t ngrid, const mpst_impute_opts* o, int32_t K, const double* u, int64_t seed, const int64_t* row_id,
                            double* x_out, double* err_out, double* seconds);

/* The distribution behind the median (get_cdfs, src/Imputation/imputation.jl:581-622; get_rdms_with_med / impute_med_and_get_cdf!,
 * src/Imputation/MPS_methods.jl:350-466; get_cdf, src/Imputation/sampling_utils.jl:205-241): the median imputer, and with it, for every
 * missing site, read off the SAME conditional distribution the median was read from - p_k = |rho phi(x_k)|^2, cdf = cumul_integrate(xs,
 * p, TrapezoidalEvenFast()), cdf /= cdf[end] -
 *   - the grid values at nq more levels: q_out[i][j][l] = x_k with k = argmin_k |cdf_k - levels[l]|, the rule MPST_IMPUTE_QUANTILE
 *     applies to a uniform number and the median applies to 0.5.  The chain is re-conditioned on the median alone, a level never
 *     feeds back.  One pass gives the quantile band (e.g. 5 % / 95 %) of every missing site of every instance;
 *   - the normalised cdf itself on the grid indices 0, s, 2s, ... and always ngrid - 1 (s = cdf_stride):
 *         ncdf = (ngrid - 2) / cdf_stride + 2      (integer division; s = 1: the whole grid, ncdf = ngrid)
 *     cdf_out[i][r][:] belongs to the r-th missing site of instance i in ASCENDING site order, whatever o->order is (the reference
 *     writes cdfs[i] by position in the conditioned MPS, MPS_methods.jl:413); rows beyond an instance's missing count are zero.
 * mpst_impute_dist is mpst_impute, mpst_impute_model_dist is mpst_impute_model_run (no u: the median draws nothing), with
 *   o->method       MPST_IMPUTE_MEDIAN; anything else: MPST_ERR_UNSUPPORTED (get_cdfs: "only supports method=:median", imputation.jl:594)
 *   nq, levels[nq]  0 <= nq <= 16, every level strictly inside (0, 1), in any order; else MPST_ERR_INVALID
 *   q_out[N][T][nq] in the encoding's domain, 0 at known sites; NULL iff nq == 0
 *   cdf_stride      0: no cdf, cdf_out NULL.  s >= 1: as above
 *   cdf_rows        rows per instance of cdf_out[N][cdf_rows][ncdf]; an instance with more missing sites: MPST_ERR_INVALID
 *   x_out, err_out, seconds  as in the sibling call.
 * Real and complex models, MPST_COMPUTE_F64 and _F32, chi_max <= 128, d <= 16.  With nq == 0 and cdf_stride == 0 the call launches
 * the kernels of the sibling call with method = median: same grids, same arithmetic, same bits.  The cdf rows are staged on the
 * device block by block (MPST_ERR_NOMEM if not even one instance fits: raise cdf_stride). */
int  mpst_impute_dist(void* ctx, int which, const uint8_t* missing, const double* grid_x, const double* grid_phi, int32_t ngrid,
                      const mpst_impute_opts* o, double* x_out, double* err_out, double* seconds, int32_t nq, const double* levels,
                      double* q_out, int32_t cdf_stride, int32_t cdf_rows, double* cdf_out);
int  mpst_impute_model_dist(void* ctx, const mpst_impute_model* m, const uint8_t* missing, const double* grid_x, const void* grid_phi,
                            int32_t ngrid, const mpst_impute_opts* o, double* x_out, double* err_out, double* seconds, int32_t nq,
                            const double* levels, double* q_out, int32_t cdf_stride, int32_t cdf_rows, double* cdf_out);

/* Marginal likelihoods: the natural log of the likelihood of the KNOWN values of every instance under every class, the missing
 * sites marginalised - what joins mpst_classify (complete series only) and the imputation engine (which conditions on the
 * known values and drops the scale).  With W_c the label slice of class c of the model AS STORED (not renormalised per class),
 * phi[i][j] the encoded value of instance i at site j and K_i its known sites,
 *     l_c(i) = sum over s_j, j not in K_i, of | < (x)_{j in K_i} phi[i][j]  (x)_{j not in K_i} e_{s_j} | W_c > |^2 :
 * a known site is projected with conj(phi), a missing site is summed over its physical index - the squared norm of what
 * precondition (src/Imputation/MPS_methods.jl:42-99) leaves behind.  Nothing missing: l_c = |yhat_c|^2, the overlap mpst_classify
 * maximises; everything missing: l_c = ||W_c||^2.  (The Born rule; not the |rho phi|^2 convention of the imputed densities.)
 *   m               as in mpst_impute_model_run; m->label_idx is ignored and may be NULL.  phi is not read at missing sites
 *                   (the host may hold NaN there).
 *   missing[N][T]   nonzero = missing; NULL = nothing missing (the same bits as an all-zero mask)
 *   logp_out[N][C]  ln l_c(i), IEEE -inf where l_c is zero; never NaN for finite inputs
 *   seconds         device time of the call, may be NULL
 * Real and complex models, MPST_COMPUTE_F64 and _F32; the chain is rescaled at every site and the logarithms of the scales are
 * accumulated in fp64 on both compute paths, so long chains neither underflow nor lose the scale.
 * MPST_ERR_INVALID: NULL m or logp_out, non-positive dimensions; MPST_ERR_UNSUPPORTED: chi_max > 128, d > 16 or C > 16. */
int  mpst_marginal_model(void* ctx, const mpst_impute_model* m, const uint8_t* missing /* [N][T], NULL = nothing missing */,
                         double* logp_out /* [N][C] */, double* seconds /* may be NULL */);

/* Leave-one-out site conditionals of COMPLETE series: for every instance i and every site t the distribution of x_t given all the
 * other values of the series, p(x_t | x_{!=t}), under the label slice c_i = m->label_idx[i] of the model (its scale is irrelevant
 * to every output).  With M_j = sum_q conj(phi[i][j][q]) W_j[:, q, :] (the projection of precondition), l_{-1} = 1,
 * l_j = l_{j-1} M_j, r_T = 1, r_j = M_j r_{j+1} (rescaled at every site: long chains do not underflow) and
 *     a_t[s] = sum_ab l_{t-1}[a] W_t[a, s, b] r_{t+1}[b],
 * the density on the grid is p_k = |sum_s conj(g_k[s]) a_t[s]|^2, g_k row k of site t's grid table: what mpst_impute_model_dist forms
 * for an instance whose only missing site is t, up to a constant factor (the conditioned state is pure, so the reference's
 * |rho phi|^2 and the Born value differ by the constant |a|^2 only).  cdf = cumul_integrate(grid_x, p, TrapezoidalEvenFast()),
 * Z = cdf[ngrid-1], F = cdf / Z.
 *   m                 as in mpst_impute_model_run (label_idx required), compute MPST_COMPUTE_F64; all of phi is read
 *   x[N][T]           the observed values, in the encoding's domain (read for pit_out only)
 *   grid_x, grid_phi, ngrid   as in mpst_impute_model_run: evenly spaced values and their states, [ngrid][d], or [T][ngrid][d] with
 *                     o->grid_per_site = 1
 *   o                 grid_per_site 0 / 1; get_err: compute err_out (else it is 0); nq levels strictly inside (0, 1), 0 <= nq <= 16;
 *                     reserved: 0
 * Outputs per (i, t), [N][T]; each may be NULL and is then skipped (at least one must be given):
 *   nll_out   -ln( |sum_s conj(phi[i][t][s]) a_t[s]|^2 / Z ): the negative log conditional density at the observed value per unit of
 *             the encoding's domain, at the exact encoded state (not the nearest grid value); +inf where the numerator is zero
 *   pit_out   F at x[i][t], linear between the two neighbouring grid values; 0 below grid_x[0], 1 above grid_x[ngrid-1]
 *   med_out   grid_x[argmin_k |F_k - 0.5|] (the median imputer's rule and tie rule)
 *   err_out   the median imputer's WMAD, weighted_median(|grid_x - med|, p / Z)
 *   q_out[N][T][nq]   grid_x[argmin_k |F_k - levels[l]|]
 * A site whose Z is not a positive finite number gives NaN in all its outputs.  seconds (may be NULL): device time of the call;
 * mpst_get_impute_phases then returns its split into (walk, grid phase).  Results do not depend on how the instances are cut into
 * blocks (by free device memory) nor on which other instances travel along.
 * MPST_ERR_INVALID: NULL m / x / grid_x / grid_phi / o, all outputs NULL, ngrid < 2, nq outside 0..16, a level outside (0, 1), q_out
 * NULL with nq > 0, label_idx NULL or out of range, grid_per_site not 0 / 1; MPST_ERR_UNSUPPORTED: MPST_COMPUTE_F32, chi_max > 128,
 * d > 16, C > 16.  A rejected call leaves the context as it was. */
typedef struct {
    int32_t grid_per_site, get_err, nq, reserved;
    const double* levels;       /* [nq] */
} mpst_sitecond_opts;
int  mpst_site_conditionals(void* ctx, const mpst_impute_model* m, const double* x /* [N][T] */, const double* grid_x, const void* grid_phi,
                            int32_t ngrid, const mpst_sitecond_opts* o, double* nll_out, double* pit_out, double* med_out, double* err_out,
                            double* q_out /* [N][T][nq] */, double* seconds /* may be NULL */);

/* Window conditionals: subsequence anomaly scores of COMPLETE series.  For every series i (class label_idx[i]), every start t and every
 * width w = 1 .. max_width with t + w <= T,
 *     nll_out[i][t][w-1] = ln l_c(i; {t, .., t+w-1}) - ln l_c(i; {}),
 * l_c(i; M) the marginal likelihood of mpst_marginal_model with the sites in M missing: -ln of the Born probability of the window's
 * values given all the others (for encodings orthonormal on the domain: the negative log conditional density per unit of domain^w).
 * One walk over each series keeps its left and right rows; each start then runs max_width steps of the density recursion, one per width.
 *   m           as in mpst_site_conditionals (label_idx required), compute MPST_COMPUTE_F64; all of phi is read
 *   max_width   1 .. T
 *   nll_out[N][T][max_width]   entries with t + w > T are NaN; +inf where the amplitude of the complete series vanishes; NaN for a width
 *               (and the wider ones of its start) whose trace or closing form is not a positive finite number.  Never NaN for a finite,
 *               non-degenerate input.
 * seconds (may be NULL): device time of the call; mpst_get_impute_phases then returns (walk, window kernel).  The result of a (series,
 * start) pair depends neither on how the instances are cut into blocks (free device memory, MPST_IMPUTE_CHUNK_GB) nor on what travels
 * along: no floating-point atomics, one reduction order.
 * MPST_ERR_INVALID: NULL m / nll_out, label_idx NULL or out of range, max_width outside 1..T, non-positive dimensions;
 * MPST_ERR_UNSUPPORTED: MPST_COMPUTE_F32, chi_max > 128, d > 16, C > 16.  A rejected call leaves the context as it was. */
int  mpst_window_conditionals(void* ctx, const mpst_impute_model* m, int32_t max_width, double* nll_out /* [N][T][max_width] */,
                              double* seconds /* may be NULL */);

/* Marginal site conditionals: the predictive distribution of every site of an INCOMPLETE series.  For instance i (class c_i =
 * m->label_idx[i], the label slice as stored - its scale cancels everywhere) with the known sites K_i = {j : missing[i][j] == 0} and
 * every site t, known or missing, the distribution of x_t given the known values of the OTHER sites, the missing ones summed over
 * their physical index.  The convention is the Born rule, that of mpst_marginal_model, mpst_window_conditionals and
 * mpst_pair_analysis (not the |rho phi|^2 of the sequential imputer; the two agree, up to a constant, only where the conditioned
 * state is pure).  With A_j[s] = W_j[:, s, :] at a missing site, M_j = sum_q conj(phi[i][j][q]) W_j[:, q, :] at a known one and the
 * density recursion of mpst_marginal_model, E' = sum_s A_j[s]^T E conj(A_j[s]) (the one term with M_j at a known site):
 *     L_{t-1}   the density over the left bond of site t, from the sites 0 .. t-1 (initial value 1),
 *     R_{t+1}   the density over its right bond, from the sites t+1 .. T-1,
 *     rho_t[s, s'] = sum_{a a' b b'} L_{t-1}[a, a'] W_t[a, s, b] conj(W_t[a', s', b']) R_{t+1}[b, b'],
 *     p_k = max(Re(sum_{s s'} conj(g_k[s]) rho_t[s, s'] g_k[s']), 0),   g_k row k of site t's grid table,
 * cdf = cumul_integrate(grid_x, p, TrapezoidalEvenFast()), Z = cdf[ngrid-1], F = cdf / Z.  Site t itself is never conditioned on; at
 * a complete series rho_t = a_t a_t^H with the a_t of mpst_site_conditionals.  L and R are rescaled to trace one at every site (long
 * chains do not underflow); no scale is returned.
 *   m                 as in mpst_site_conditionals (label_idx required), compute MPST_COMPUTE_F64; phi[i][j] is read at the known sites
 *                     and at a missing site only when x[i][j] is finite
 *   missing[N][T]     non-zero: the site is missing; NULL: nothing is missing
 *   x[N][T]           the values in the encoding's domain: the observed one at a known site, at a missing site the held-out true value or
 *                     NaN; NULL: no value anywhere (pit_out must then be NULL, nll_out is given at the known sites only)
 *   grid_x, grid_phi, ngrid, o   as in mpst_site_conditionals
 * Outputs per (i, t), [N][T]; each may be NULL and is then skipped (at least one must be given):
 *   med_out, err_out, q_out[N][T][nq]   as in mpst_site_conditionals, rules and tie rules included
 *   mean_out  trapezoid(grid_x * p) / Z
 *   nll_out   -ln(phi[i][t]^H rho_t phi[i][t] / Z), at the exact encoded state; +inf where the numerator is not positive
 *   pit_out   F at x[i][t], linear between the two neighbouring grid values; 0 below grid_x[0], 1 above grid_x[ngrid-1]
 * nll_out and pit_out are produced wherever x[i][t] is finite: at a known site they are leave-one-out scores with the missing sites
 * summed out, at a missing site held-out scores of the value the caller supplied; elsewhere they are NaN.  A site whose Z is not a
 * positive finite number gives NaN in all its outputs.  Never NaN for finite, non-degenerate input.
 * seconds (may be NULL): device time of the call; mpst_get_impute_phases then returns (walk, grid phase).  The result of an (instance,
 * site) pair depends neither on how the instances are cut into blocks (free device memory, MPST_IMPUTE_CHUNK_GB) nor on what travels
 * along: no floating-point atomics, one reduction order.
 * MPST_ERR_INVALID: NULL m / grid_x / grid_phi / o, all outputs NULL, pit_out without x, ngrid < 2, nq outside 0..16, a level outside
 * (0, 1), q_out NULL with nq > 0, label_idx NULL or out of range, grid_per_site not 0 / 1; MPST_ERR_UNSUPPORTED: MPST_COMPUTE_F32,
 * chi_max > 128, d > 16, C > 16.  A rejected call leaves the context as it was. */
int  mpst_marginal_conditionals(void* ctx, const mpst_impute_model* m, const uint8_t* missing /* [N][T], NULL = nothing missing */,
                                const double* x /* [N][T] */, const double* grid_x, const void* grid_phi, int32_t ngrid,
                                const mpst_sitecond_opts* o, double* nll_out, double* pit_out, double* med_out, double* err_out,
                                double* mean_out, double* q_out /* [N][T][nq] */, double* seconds /* may be NULL */);

/* Entanglement analysis (src/Analysis/analyse.jl) of a real model (dtype MPST_DTYPE_F64, compute MPST_COMPUTE_F64; complex
 * models: MPST_ERR_UNSUPPORTED, the reference cannot analyse them either), chi_max <= 128, d <= 16.  Every class MPS is the
 * label slice of class c, normalised (expand_label_index, utils.jl:356-370).  Natural log throughout.
 * bipartite_spectrum / single_site_spectrum (analyse.jl:47-64, :122-138) on the model of m (m->N, m->phi, m->label_idx unused):
 * bee_out[C][T] (entry T-1 repeats bond T-2, as the reference's last cut does), see_out[C][T]; either may be NULL. */
int  mpst_entanglement(void* ctx, const mpst_impute_model* m, double* bee_out, double* see_out);
/* see_variation (analyse.jl:168-194) for class cls on the m->N encoded series m->phi [N][T][d]: out[N][T][T] = [instance][k][site],
 * the single-site entropies after sites 0..k-1 were measured at the instance's values (row 0: single_site_spectrum; zero at
 * sites < k; NaN rows where the measured state vanishes).  m->label_idx is ignored.  seconds (may be NULL) = device time.
 * MPST_ERR_DOMAIN names the class, instance, k, site and offending value in mpst_last_error. */
int  mpst_see_variation(void* ctx, const mpst_impute_model* m, int32_t cls, double* out, double* seconds);
/* Pair analysis of every class MPS (m->N, m->phi, m->label_idx unused): the two-site reduced density matrix rho_ij of every pair of
 * sites i < j, the physical index of every other site summed out (the convention of mpst_marginal_model; the model's distribution for
 * encodings orthonormal on the domain).  Entropies S(rho) = -sum over eigenvalues lam > 0 of lam ln lam (of (rho + rho^T) / 2; no
 * rho_correct, no threshold, no MPST_ERR_DOMAIN).  Each output may be NULL:
 *   mi_out[C][T][T]   symmetric; [i][j] = S(rho_i) + S(rho_j) - S(rho_ij) off the diagonal, S(rho_i) on it;
 *   mean_out[C][T]    tr(rho_i O_i), O a real symmetric observable: obs[d][d] (obs_per_site 0) or obs[T][d][d] (1), row-major;
 *   cov_out[C][T][T]  symmetric; tr(rho_ij (O_i (x) O_j)) - mean_i mean_j off the diagonal, tr(rho_i O_i O_i) - mean_i^2 on it.
 * A class whose state is zero gives NaN in its slices.  seconds (may be NULL) = device time; mpst_get_impute_phases then gives
 * (the pair walk k_an_pair, the entropy kernel k_an_pair_ent).  Results do not depend on the free device memory or MPST_IMPUTE_CHUNK_GB.
 * MPST_ERR_INVALID: all three outputs NULL, mean_out or cov_out with obs NULL, obs_per_site not 0 / 1; MPST_ERR_UNSUPPORTED: a complex
 * model, MPST_COMPUTE_F32, chi_max > 128, d > 16, mi_out with d > 11 (the pair matrix is d^2 x d^2 and the in-workgroup Jacobi holds
 * n <= 128; the moments have no such limit).  A rejected call leaves the context as it was. */
int  mpst_pair_analysis(void* ctx, const mpst_impute_model* m, const double* obs /* [d][d] or [T][d][d]; NULL: no moments */,
                        int32_t obs_per_site, double* mi_out /* [C][T][T] */, double* mean_out /* [C][T] */,
                        double* cov_out /* [C][T][T] */, double* seconds /* may be NULL */);
/* Model overlaps: the inner products of the class states of K models.  With psi_{k,c} the label slice c of model k AS STORED (not
 * renormalised), G_ab[c, c'] = <psi_{a,c} | psi_{b,c'}> = sum_s conj(psi_{a,c}(s)) psi_{b,c'}(s) for every requested pair (a, b).  The
 * models agree in T, d, label_site and dtype; their bond dimensions and C may differ.  models[k] is read as mpst_entanglement reads its
 * model (N, phi, label_idx unused); real and complex models, compute MPST_COMPUTE_F64.
 *   pairs[P][2]   indices (a, b) into models; NULL: every a <= b in row order ((0,0), (0,1), .., (1,1), ..), K (K + 1) / 2 of them, P ignored
 *   g_out[P][Cmax][Cmax], lg_out[P]   Cmax = max_k C_k.  Entry [c][c'] of pair p is G_ab[c, c'] = g exp(lg_out[p]), conjugate on a;
 *                 (re, im) pairs of doubles for MPST_DTYPE_C64; entries beyond C_a x C_b are zero.  The environments are rescaled by an exact
 *                 power of two at every site and the exponent is kept per pair, so chains of any length neither underflow nor lose bits.
 *                 An environment that is exactly zero, or a G that is: g = 0, lg = -INFINITY.  Finite inputs never give NaN.
 *   seconds       device time of the call, may be NULL
 * The result of a pair depends neither on which other pairs travel along, nor on their order, nor on how the pairs are cut into blocks
 * (by free device memory or MPST_IMPUTE_CHUNK_GB): no floating-point atomics, one reduction order.
 * MPST_ERR_INVALID: NULL models / g_out / lg_out, K < 1, a pair index outside [0, K), models that disagree in T, d, label_site or dtype;
 * MPST_ERR_UNSUPPORTED: MPST_COMPUTE_F32, chi_max > 128, d > 16, d chi_max > 1024, C > 16.  A rejected call leaves the context as it was. */
int  mpst_model_overlaps(void* ctx, const mpst_impute_model* models /* [K] */, int32_t K,
                         const int32_t* pairs /* [P][2]; NULL: every a <= b, row order, P ignored */, int32_t P,
                         double* g_out /* [P][Cmax][Cmax], (re, im) pairs for MPST_DTYPE_C64 */,
                         double* lg_out /* [P] */, double* seconds /* may be NULL */);

/* normalize!(W), RealRealHighDimension.jl:852. */
/* Device seconds of the last imputation call split into its two kernels: [0] the environment pass (k_imp_right, MFMA),
 * [1] the sweep with the densities and selections (k_imp_left).  After mpst_site_conditionals: (walk, grid phase); after
 * mpst_window_conditionals: (walk, window kernel); after mpst_marginal_conditionals: (walk, grid phase); after
 * mpst_marginal_model, which has one kernel: (its device seconds, 0); after mpst_pair_analysis: (pair walk, entropy kernel); after
 * mpst_prefix_marginals: (environment kernel k_prefix_env, walk-and-score kernel k_prefix_score); after mpst_segment_marginals: (the two
 * table kernels k_segment_left and k_prefix_env, the walk kernel k_segment_walk); after mpst_rolling_forecasts: (tables + rows + score,
 * grid phase); after mpst_observed_conditionals: (operators + walk, grid phase). */
int  mpst_get_impute_phases(void* ctx, double* seconds_out /*[2]*/);
/* How the last imputation call ran (at most n entries): out[0] = 1 when the grid states were recognised as the Fourier basis
 * (src/Encodings/bases.jl:23-42) on a uniform grid and the conditional densities |rho phi(x)|^2 and their cumulative trapezoid
 * (src/Imputation/sampling_utils.jl:162-199) were evaluated in closed form instead of from the table of grid states;
 * out[1] = 1 when the sweep over the sites (impute_at!, src/Imputation/MPS_methods.jl:103-177) ran for sixteen instances per
 * workgroup (closed-form densities and panels that fit the LDS; otherwise one instance per workgroup - same results);
 * out[2] = the workgroups of the environment pass (one per instance, whatever the number of trajectories), out[3] = the chains
 * (instance, trajectory) the sweep ran for.  After mpst_segment_marginals: out[0] = out[1] = 0, out[2] = the blocks of series its walk
 * kernel was launched for, out[3] = the (series, start) items it walked.  After mpst_rolling_forecasts: out[0] = out[1] = 0, out[2] = the
 * blocks of series, out[3] = the blocks of targets the chains of a block of series were cut into. */
int  mpst_get_impute_info(void* ctx, int32_t* out, int32_t n);

int  mpst_normalize(void* ctx);

/* Diagnostics used by bench.py / tests (no reference counterpart). */
int  mpst_selftest_mfma(void* ctx, const double* A /*16xK row-major*/, const double* B /*Kx16*/,
                        int32_t K, double* C_out /*16x16*/);
/* mpst_selftest_eig: one solve of the bond eigensolver on a symmetric positive semi-definite G.  n <= 128 runs the solver of the
 * fused chain, larger n the large-bond solvers.  lambda_out descending; column k of E_out is vector k; *sweeps reports the route:
 * -1 tridiagonal route, verified on the device; 0 tridiagonal route rejected by its verification, Jacobi delivered; > 0 Jacobi
 * asked for, its sweeps; n > 128: -3 blocked solver verified, -2 multi-workgroup Jacobi.  Delivered: the min(n, 32) largest pairs on
 * the tridiagonal route (bit 3: min(n, 64)), everything on a Jacobi route (zero vectors for zero eigenvalues), min(n, 128) pairs
 * above 128; the rest of lambda_out / E_out is zero.  The bits of alg:
 *   bits 0-1  0 tridiagonal route with its fallback, 1 (MPST_SVD_JACOBI) Jacobi alone; n > 128: 0 blocked solver, the Jacobi
 *             solver if its verification asks for it, 2 the Jacobi solver alone.
 *   bit 2 (4)   pair mode, n even: G = [[A, -B], [B, A]] is the real embedding of the Hermitian A + iB, whose every eigenvalue G has
 *             twice.  One vector u per pair is computed; column 2k holds u, column 2k + 1 its partner J u = (-u_im, u_re), and
 *             lambda_out[2k] = lambda_out[2k + 1].
 *   bit 3 (8)   n <= 128: up to 64 eigenpairs instead of 32 (what a bond with chi_max up to 64 asks for), of which the vectors of
 *             pairs above 1e-13 of the largest are verified and delivered (the rule of the subspace solver's Rayleigh-Ritz problem).
 *   bit 4 (16)  n <= 128: through the gated launcher of that Rayleigh-Ritz problem (always the tridiagonal route with 64 pairs, so bit
 *             3 is implied and bits 0-2 must be 0), its gate word set to 1.
 *   bit 5 (32)  with bit 4: gate word 0.  lambda_out, E_out and *sweeps are filled with -7 (-7.0) on the device beforehand and must
 *             come back so: a closed gate makes both launches leave at once.
 * MPST_ERR_INVALID: bit 3 or 4 with n > 128, bit 5 without bit 4, bit 4 with any of bits 0-2, any higher bit. */
int  mpst_selftest_eig(void* ctx, const double* G /*n*n symmetric*/, int32_t n, int32_t alg,
                       double* lambda_out /*n*/, double* E_out /*n*n row-major [i][k]*/, int32_t* sweeps);
/* Per-kernel timing with HIP events recorded on the engine's own stream around every launch
 * of the selected kernel classes during mpst_sweep / mpst_bond_step (bit k of kernel_mask):
 * 0 yhat, 1 grad (fused chain: yhat + gradient partials), 2 grad_reduce + update, 3 gram (fused chain: with the optimiser
 * step), 4 eig_tri (default chain: k_eig_trivec, tridiagonalisation + eigenvectors; large-bond path: the whole eigensolver), 5 split, 6 env (fused chain: + back-split + next
 * bond tensor), 7 bt_assemble, 8 all-reduce, 9 eig_vec (only with MPST_EIG_SPLIT=1), 10 eig_fin.
 * mpst_set_profile also resets the accumulators; mpst_get_profile returns the summed device
 * microseconds and the launch count per class (arrays of 16). */
int  mpst_set_profile(void* ctx, uint32_t kernel_mask);
int  mpst_get_profile(void* ctx, double* total_us /*[16]*/, int64_t* count /*[16]*/);
/* which launch chain the context resolved to for its current sizes / options: out[0] fused chain (bond tensors up to
 * 128 x 128, 6 launches per bond), out[1] large-bond path (d*chi_max > 128), out[2] partial gradients per optimiser step
 * of the fused chain, out[3] 64-series chunks of the unfused chain, out[4] capacity bond dimension, out[5] ranks,
 * out[6] sweeps replayed from a hipGraph, out[7] bonds on which the blocked large-bond eigensolver handed over to the
 * library solver, out[8] bonds whose persistent tridiagonalisation gave up waiting for its peers and was redone one
 * launch per step, out[9] bonds whose XCD-local tridiagonalisation found its workgroups on more than one XCD and was
 * redone with the cross-XCD exchange, out[10] the fused chain runs the sliced bond GEMMs (k_yhat_s + k_grad_s: no partial
 * gradients per workgroup), out[11] shares per gradient block of k_grad_s, out[12] the tridiagonalisation and the
 * eigenvectors of a bond run in one launch (k_eig_trivec), out[13] large-bond sweeps that were redone bond by bond because
 * a bond's on-device verification failed, out[14] large bonds: the eigensolver's verdict is read once per sweep instead of
 * once per bond (no host synchronisation inside a sweep), out[15] 0, or 1 + dtype when the element-typed kernels
 * (csrc/mpst_typed.hip) run the sweep */
int  mpst_get_info(void* ctx, int32_t* out /*[16]*/);
/* the same, at most n entries: for callers compiled against another revision of this header.  Entries beyond the 16 of mpst_get_info:
 * out[16] large bonds the randomised subspace eigensolver attempted (real AND complex element types, d*chi_max > 128: top-chi_max
 * singular triplets of the bond matrix by five GEMM half-steps + a (chi_max + 32)-dimensional Rayleigh-Ritz problem, certified on
 * the device against the Gram matrix), out[17] those whose result was accepted - the others were solved by the exact Householder
 * path.  Both counters are as of the last sweep, batch or bond step that RETURNED (they are read at that call's own synchronisation
 * point; the query does not wait for the stream), out[18] the bonds of a sweep run FOUR launches (k_grad_s, k_gram_upd, k_eig_trivec, k_bond_tail: verification +
 * polish of the eigenvectors, back-split, update_caches!, the next bond's tensor and the next bond's overlaps in the last one;
 * Float64, KLD, d*chi_max <= 128, chi_max <= 32, one rank, update_iters = 1, no track_cost), out[19] sweeps / bond steps in which a
 * tail launch's verification failed and the rest ran on the six-launch chain (whose k_eig_fin has the Jacobi fallback), out[20] on
 * the four-launch chain the part of the tail that needs no eigenvector (the dense S tile of every 16-series tile, the next bond's
 * overlap product) is formed by side workgroups of the k_eig_trivec launch and read back by k_bond_tail (0: MPST_TAIL_PRE=0, the
 * tail forms both itself; the same bits either way), out[21] with rebuild_caches the two construct_caches of a sweep are hidden beside
 * the eigensolver: the side workgroups of every k_eig_trivec launch rebuild one environment row of a site that is already final, and a
 * walk of two steps closes each half-sweep (needs out[20] and the one-launch walk; 0: MPST_REBUILD_SIDE=0 or rebuild_caches off - the
 * full walks; the same bits either way), out[22] rows rebuilt that way in the last sweep that returned: 2 max(0, T - 3) where out[21]. */
int  mpst_get_info_n(void* ctx, int32_t* out, int32_t n);
/* in-kernel phase times (us) of the last eigensolver launch: tridiagonalisation, bisection,
 * tridiagonal eigenvectors, back-transformation, verification+re-orthonormalisation; us[5] = shader
 * cycles (s_memtime) of the tridiagonalisation, for the effective clock */
int  mpst_get_eig_phases(void* ctx, double* us /*[6]*/);
/* in-kernel phase stamps (us since workgroup 0 started; -1: not taken) of the last stamped k_bond_tail launch - the four-launch chain's
 * last launch, which stands for k_eig_fin + update_caches! + the back-split (RealRealHighDimension.jl:107-203) and the next bond's
 * yhat pass (loss_functions.jl:248-262).  Which bond leaves stamps: MPST_TAIL_STAMP="lid,going_left" (default: the middle bond of the
 * backward half-sweep).  us[0..15] workgroup 0, which also hosts a job of the next bond's tensor when the sweep goes on: start,
 * candidate vectors requested, the side workgroups' results requested, bond dimensions known, everything requested, trace pieces
 * published, truncation rule, candidates and S tile in LDS, verified + polished, role operands requested, new environment rows,
 * z + row dot, tile done, role done, stores drained (15 stamps).  With MPST_TAIL_PRE=0 the tail forms the S tile and the overlap
 * product itself and the sequence is the longer one: start, candidate vectors requested, factors requested, bond dimensions known,
 * everything requested, factors in LDS, truncation rule, candidates in LDS, verified + polished, overlap product issued, role operands
 * requested, barrier B1 passed, dense S tile formed, new environment rows, z + row dot, tile done (a role host's last two stamps,
 * role done and stores drained, do not fit the 16 slots and are not kept); us[16..31] the same for the last workgroup (a tile, no
 * role); us[32..35] the side workgroups of that bond's k_eig_trivec launch (out[20] of mpst_get_info_n): how many, earliest start,
 * latest start, latest end - negative, that launch precedes the tail; us[48..51] bonds since the context was created
 * by how far from orthonormal their candidate vectors were: |Z^T Z - I| below 1e-13 (nothing to do), below 1e-8 (first-order polish),
 * below 3e-5 (second-order), above (two passes); us[52], us[53], us[54] the earliest start, the latest end and the latest start over
 * ALL workgroups of the stamped launch */
int  mpst_get_tail_phases(void* ctx, double* us /*[55]*/);

/* Prefix marginals: for every series i, every prefix length t = 0 .. T and every class c the log likelihood of the first t values with
 * the sites t .. T-1 summed out - what mpst_marginal_model gives for the suffix mask of t (missing[i][j] = j >= t), for all T + 1 masks
 * from one walk per series:
 *     logp_out[i][t][c] = ln l_c(i; t),   l_c(i; t) = x_t G_c^t x_t^H,
 * x_t the row walk through the known sites 0 .. t-1 and G_c^t the density recursion from the right end through the sites T-1 .. t, which
 * depends on the model only and is computed once per call.  Index 0 is ln ||W_c||^2 for every series, index T the complete series.
 * m as in mpst_marginal_model: the label slice of the model AS STORED; label_idx is not read, all of phi is; real and complex models,
 * compute MPST_COMPUTE_F64.  A likelihood that is zero (or not finite) is -INFINITY; if it is the walk of a series that vanished at
 * site j, every prefix longer than j of that series is -INFINITY.  Never NaN.  A series gives the same bits whichever series travel with
 * it and however the series are cut into blocks (free device memory, MPST_IMPUTE_CHUNK_GB).  seconds (may be NULL) = device time;
 * mpst_get_impute_phases then gives (environment kernel, walk-and-score kernel).
 * MPST_ERR_INVALID: NULL m / logp_out, a malformed model; MPST_ERR_UNSUPPORTED: compute other than MPST_COMPUTE_F64, chi_max > 128,
 * d > 16, C > 16; MPST_ERR_NOMEM: the (label_site + 1) C + (T - label_site) tables of chi_max^2 elements do not fit the query budget - they
 * are not cut over t.  A rejected call leaves the context as it was. */
int  mpst_prefix_marginals(void* ctx, const mpst_impute_model* m, double* logp_out /* [N][T+1][C] */, double* seconds /* may be NULL */);

/* Segment marginals: for every series i, every class c, every start a and every width w = 1 .. max_width with a + w <= T the log
 * likelihood of the values of the sites a .. a+w-1 ALONE, every other site summed out - what mpst_marginal_model gives for the mask that
 * is set everywhere but on the segment:
 *     logp_out[i][a][w-1][c] = ln l_c(i; a, w),   l_c(i; a, w) = Re sum_xy E[x][y] G_c^{a+w}[x][y],
 * E the walk from the table entry L^a through the known sites a .. a+w-1, E <- M_j^T E conj(M_j), M_j = sum_q conj(phi[i][j][q])
 * W_j[:, q, :]; L^t the density recursion of mpst_marginal_model from the left end through the sites 0 .. t-1 and G^t the one from the
 * right end through T-1 .. t, all of them missing.  Both tables depend on the model only and are computed once per call; a series costs
 * T * max_width known-site steps, whatever T - w is.
 *   m           as in mpst_marginal_model: the label slice of the model AS STORED; label_idx is not read, all of phi is; real and complex
 *               models, compute MPST_COMPUTE_F64
 *   max_width   1 .. T
 *   logp_out[N][T][max_width][C]   entries with a + w > T are NaN.  An entry is -INFINITY where a closing form or the trace of a step is
 *               not a positive finite number, and so is every wider entry of that start: for all classes while the walk is left of the
 *               label site, for the class at hand from the label site on.  A table chain that vanishes gives -INFINITY wherever it is
 *               needed.  Never NaN inside the triangle for finite input.
 *   lnorm_out[C]   ln ||W_c||^2, what subtracting gives the likelihood under the normalised class state; may be NULL
 * seconds (may be NULL): device time of the call; mpst_get_impute_phases then returns (table kernels, walk kernel).  The result of a
 * (series, start) pair depends neither on how the series are cut into blocks (free device memory, MPST_IMPUTE_CHUNK_GB) nor on what
 * travels along: no floating-point atomics, one reduction order.
 * MPST_ERR_INVALID: NULL m / logp_out, max_width outside 1..T, a malformed model; MPST_ERR_UNSUPPORTED: compute other than
 * MPST_COMPUTE_F64, chi_max > 128, d > 16, C > 16; MPST_ERR_NOMEM: the (T + 1)(C + 1) tables of chi_max^2 elements (and beyond the LDS
 * limit the scratch of the walk's resident workgroups) do not fit the query budget - they are not cut.  A rejected call leaves the
 * context as it was. */
int  mpst_segment_marginals(void* ctx, const mpst_impute_model* m, int32_t max_width, double* logp_out /* [N][T][max_width][C] */,
                            double* lnorm_out /* [C], may be NULL */, double* seconds /* may be NULL */);

/* Rolling-origin forecasts: for every COMPLETE series i, every origin t = 0 .. T-1 and every horizon h = 1 .. max_horizon with
 * u = t + h - 1 < T the predictive distribution of x_u given x_0 .. x_{t-1} ONLY, every site from t on but u summed over its physical
 * index - what mpst_marginal_conditionals gives at site u for the suffix mask of t (missing[i][j] = j >= t), for all origins from one
 * row walk per series against model-only tables:
 *     rho_c[s, s'] = x_t K_c^{t,u}[s, s'] x_t^H,   K_c^{u,u}[s, s'] = W_u[:, s, :] G_c^{u+1} W_u[:, s', :]^H,
 *     K_c^{t,u}[s, s'] = sum_q W_t[:, q, :] K_c^{t+1,u}[s, s'] W_t[:, q, :]^H,
 * x_t the walk of mpst_prefix_marginals through the sites 0 .. t-1 and G its table; then p_k = max(Re(g_k^H rho g_k), 0) on the grid
 * states of site u and everything as in mpst_marginal_conditionals.
 *   m           as in mpst_marginal_conditionals, all of phi is read; label_idx[i] = c in 0 .. C-1: rho = rho_c under the label slice c as
 *               stored; label_idx[i] = -1: the class mixture rho = sum_c rho_c with every class at its stored scale, i.e. weighted by the
 *               likelihood of the first t values under it (the posterior of mpst_prefix_marginals at length t); real and complex models,
 *               compute MPST_COMPUTE_F64
 *   max_horizon 1 .. T
 *   x[N][T]     the observed values for pit_out (encoding domain); NULL: no pit
 *   grid_x, grid_phi, ngrid, o   as in mpst_site_conditionals; a per-site table is read at the target u
 *   outputs [N][T][max_horizon], entry [i][t][h-1], each may be NULL: nll_out (-ln of the density of the encoded state of x_u, +INFINITY
 *               where its numerator is not positive), pit_out (the cdf at x[i][u]), med_out, err_out (WMAD), mean_out,
 *               q_out[N][T][max_horizon][nq].  Exactly NaN where t + h > T; NaN in every output of a triple whose normalisation is not a
 *               positive finite number - every origin > j of a series whose encoded state at site j is all zero; never NaN otherwise.
 * seconds (may be NULL): device time of the call; mpst_get_impute_phases then returns (tables + rows + score, grid phase) and
 * mpst_get_impute_info out[2] = the blocks of series, out[3] = the blocks of targets of a block of series.  The result of a triple
 * depends neither on how the series and the targets are cut into blocks (free device memory, MPST_IMPUTE_CHUNK_GB) nor on what travels
 * along: no floating-point atomics, one reduction order.
 * MPST_ERR_INVALID: NULL m / grid / o, every output NULL, pit_out without x, ngrid < 2, bad levels, max_horizon outside 1..T, label_idx
 * outside -1 .. C-1, a malformed model; MPST_ERR_UNSUPPORTED: MPST_COMPUTE_F32, chi_max > 128, d > 16, C > 16; MPST_ERR_NOMEM: G / lnG
 * and the table kernel's scratch do not fit the query budget - they are not cut.  A rejected call leaves the context as it was. */
int  mpst_rolling_forecasts(void* ctx, const mpst_impute_model* m, int32_t max_horizon, const double* x /* [N][T], NULL: no pit */,
                            const double* grid_x, const void* grid_phi, int32_t ngrid, const mpst_sitecond_opts* o,
                            double* nll_out, double* pit_out, double* med_out, double* err_out, double* mean_out,
                            double* q_out /* [N][T][H][nq] */, double* seconds);

/* Observed conditionals: mpst_marginal_conditionals with a MEASUREMENT at every site in place of "known exactly" / "missing" (DESIGN.md
 * 29).  Site (i, t) has a kind and two parameters a[i][t], b[i][t] in the encoding's domain:
 *     MPST_OBS_EXACT     the value is x[i][t], state phi[i][t]                  E = phi phi^H
 *     MPST_OBS_MISSING   nothing observed                                       E = 1
 *     MPST_OBS_GAUSS     y = a, noise sd b > 0:  k_k = exp(-(x_k - a)^2 / (2 b^2)) / (b sqrt(2 pi))
 *     MPST_OBS_INTERVAL  a <= x <= b:            k_k = 1 if a <= x_k <= b (as doubles), else 0
 *                                                                               E[s, s'] = sum_k w_k k_k g_k[s] conj(g_k[s'])
 *     MPST_OBS_OPERATOR  the caller's Hermitian d x d matrix                    E = E_user[i][t]
 * w_k the weights of cumul_trapz_even on the grid (dx / 2 at the two ends, dx inside), g_k row k of site t's grid table.  The density
 * walk steps through a site with operator E as L' = sum_{s'} B_{s'}^T L conj(A_{s'}), B_{s'} = sum_s conj(E[s, s']) A_s, A_s =
 * W_t[:, s, :] (and alike from the right); rho_t, p_k, Z and the selection rules are those of mpst_marginal_conditionals - site t's own
 * observation never enters rho_t.
 *   m, grid_x, grid_phi, ngrid, o   as in mpst_marginal_conditionals; phi[i][t] is read at the EXACT sites, and at a MISSING site only
 *                     when x[i][t] is finite
 *   kind[N][T]        MPST_OBS_*; NULL: every site EXACT
 *   a, b [N][T]       read at the GAUSS and INTERVAL sites only; may be NULL when there are none
 *   E_user[N][T][d][d]   row-major, (re, im) pairs for MPST_DTYPE_C64; read at the OPERATOR sites only; may be NULL when there are none
 *   x[N][T]           the value of an EXACT site, the held-out true value of a MISSING one or NaN; NULL: no value anywhere (pit must
 *                     then be NULL, nll_obs of an EXACT site is still given)
 * Outputs (mpst_observed_out), each may be NULL and is then skipped, at least one must be given.  Per (i, t), [N][T]:
 *   pred_med, pred_err, pred_mean, pred_q[N][T][nq]   median, WMAD, mean and levels of p: the true value given the OTHER sites' observations
 *   post_med, post_err, post_mean, post_q[N][T][nq]   the same of k_k p_k: the true value given ALL observations.  Equal to the predictive
 *                     group at a MISSING site; NaN at EXACT and OPERATOR sites and where trapz(k p) is not a positive finite number
 *   nll_obs           -ln(tr(E_t rho_t) / Z), the leave-one-out score of the observation as it was made: at an EXACT site the nll of
 *                     mpst_marginal_conditionals; at a MISSING site the held-out score of a finite x[i][t], else NaN; +inf where the
 *                     numerator is not positive
 *   pit               at EXACT sites (and at a MISSING site with a finite x[i][t]) as in mpst_marginal_conditionals; NaN elsewhere
 * Per series: logev[N], the natural log of the un-normalised chain value under class label_idx[i] - the logs of the traces the left
 * walk divides by plus ln tr(E_{T-1} rho_{T-1}); ln ||W_c||^2 for a row of MISSING sites; -inf where a trace is not a positive finite
 * number.  E_out[N][T][d][d] (layout of E_user): the operators the walk used, EXACT and MISSING sites written as phi phi^H and 1.
 * seconds (may be NULL): device time; mpst_get_impute_phases then returns (operators + walk, grid phase).  Results depend neither on how
 * the series are cut into blocks nor on what travels along: no floating-point atomics, one reduction order.
 * MPST_ERR_INVALID: what mpst_marginal_conditionals refuses, and: out NULL or every output NULL, a kind outside 0 .. 4, GAUSS with b not
 * a positive finite number or a not finite, INTERVAL with a > b or an end that is not finite, a GAUSS / INTERVAL site with a or b NULL,
 * an OPERATOR site with E_user NULL; MPST_ERR_UNSUPPORTED as there.  A rejected call leaves the context as it was. */
enum { MPST_OBS_EXACT = 0, MPST_OBS_MISSING = 1, MPST_OBS_GAUSS = 2, MPST_OBS_INTERVAL = 3, MPST_OBS_OPERATOR = 4 };
typedef struct {
    double* pred_med;
    double* pred_err;
    double* pred_mean;
    double* pred_q;     /* [N][T][nq] */
    double* post_med;
    double* post_err;
    double* post_mean;
    double* post_q;     /* [N][T][nq] */
    double* nll_obs;
    double* pit;
    double* logev;      /* [N] */
    void* E_out;        /* [N][T][d][d] */
} mpst_observed_out;
int  mpst_observed_conditionals(void* ctx, const mpst_impute_model* m, const uint8_t* kind /* [N][T], NULL = all EXACT */,
                                const double* a, const double* b /* [N][T] */,
                                const void* E_user /* [N][T][d][d], read at OPERATOR sites only, may be NULL */,
                                const double* x /* [N][T] */, const double* grid_x, const void* grid_phi, int32_t ngrid,
                                const mpst_sitecond_opts* o, mpst_observed_out* out, double* seconds /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MPSTIME_HIP_H */
