// C ABI of libmpstime_hip.so (include/mpstime_hip.h): context management, host<->device
// marshalling, the sweep driver (src/Training/RealRealHighDimension.jl:724-851 restated as a
// stream of kernel launches with no host read-back inside a sweep) and the RCCL plumbing.
#include <rccl/rccl.h>
#include <dlfcn.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include "mpst_internal.h"
#include "mpst_batch_groups.h"
#include "mpst_bond_plan.h"
#include "mpst_prefix_plan.h"
#include "mpst_segment_plan.h"
#include "mpst_rolling_plan.h"
#include "mpst_observed_plan.h"

using namespace mpst;

namespace {

thread_local std::string g_err;  // errors raised without a context (mpst_create)

// ---- RCCL, bound at run time ----------------------------------------------------------------------------------------------
// The library is NOT linked against librccl: a host process that has imported torch already holds torch's own copy
// (torch/lib/librccl.so, same SONAME librccl.so.1 as /opt/rocm/lib's), and two copies of a collective library in one process
// - two sets of bootstrap threads, IPC registries and topology caches - is a hazard on first multi-GPU contact.  Order:
// MPST_RCCL_LIB (explicit path), then whatever librccl.so.1 the process has ALREADY loaded (RTLD_NOLOAD: the host's copy
// wins), then the system one.  mpst_comm_init compares the version of the bound library with the header this file was
// compiled against (same major version, see there) and mpst_comm_library reports path and version.
struct Rccl {
    void* h = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGetVersion) GetVersion = nullptr;
    int version = 0;
    std::string path, how, err;
};
void rccl_load(Rccl& r) {
    const char* envp = getenv("MPST_RCCL_LIB");
    if (envp && !*envp) envp = nullptr;                // an empty value means unset
    if (envp) {
        r.h = dlopen(envp, RTLD_NOW | RTLD_LOCAL);
        r.how = "MPST_RCCL_LIB";
    }
    if (!r.h && !envp) {
        for (const char* nm : {"librccl.so.1", "librccl.so"}) {
            if ((r.h = dlopen(nm, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD))) { r.how = "already loaded by the host process"; break; }
        }
    }
    if (!r.h && !envp) {
        for (const char* nm : {"/opt/rocm/lib/librccl.so.1", "librccl.so.1", "librccl.so"}) {
            (void)dlerror();                           // the message reported below belongs to the last attempt, not to the probes above
            if ((r.h = dlopen(nm, RTLD_NOW | RTLD_LOCAL))) { r.how = "system library"; break; }
        }
    }
    if (!r.h) {
        const char* de = dlerror();
        r.err = std::string("librccl could not be loaded: ") + (de ? de : "not found");
        return;
    }
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.h, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.h, "ncclCommDestroy");
    r.AllReduce = (decltype(r.AllReduce))dlsym(r.h, "ncclAllReduce");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.h, "ncclGetErrorString");
    r.GetVersion = (decltype(r.GetVersion))dlsym(r.h, "ncclGetVersion");
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllReduce || !r.GetErrorString || !r.GetVersion) {
        r.err = "librccl lacks a required entry point";
        r.h = nullptr;
        return;
    }
    Dl_info di;
    if (dladdr((void*)r.AllReduce, &di) && di.dli_fname) r.path = di.dli_fname;
    (void)r.GetVersion(&r.version);
}
// one-time, thread-safe: contexts on different threads may call mpst_comm_init / mpst_comm_library concurrently
Rccl* rccl_get() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] { rccl_load(r); });
    return &r;
}
// the entry points of the bound library, or null with the reason in *why
Rccl* rccl_ready(std::string* why) {
    Rccl* r = rccl_get();
    if (!r->h) {
        if (why) *why = r->err;
        return nullptr;
    }
    return r;
}

enum KClass { K_YHAT = 0, K_GRAD, K_UPDATE, K_GRAM, K_EIG_TRI, K_SPLIT, K_ENV, K_BT, K_ALLREDUCE, K_EIG_VEC, K_EIG_FIN, K_NCLASS };

using DevStream = DevOwned<hipStream_t, hipStream_t, hipStreamDestroy>;
using DevGraphExec = DevOwned<hipGraphExec_t, hipGraphExec_t, hipGraphExecDestroy>;
inline hipError_t release_big(BigEig* b) { big_eig_destroy(b); return hipSuccess; }
inline hipError_t release_blocked(BlockedEig* b) { blocked_eig_destroy(b); return hipSuccess; }

struct Ctx;

// ---- the device memory of a context, grouped by the event that replaces it (released first, built aside, moved in complete) ---
// The MPS: replaced by mpst_set_mps when the capacity changes.
struct Mps {
    int cap = 0;              // capacity bond dimension of all device buffers
    int64_t site_stride = 0;
    DevBuf<double> sites;     // (E) T slots of site_stride elements
    DevBuf<int32_t> chi;         // device [T+1]
    DevBuf<int32_t> label_site;  // device
};

// Large bonds, sweeps: the state an optimistic sweep starts from, so that a sweep in which any bond failed can be redone bond by bond
struct Snapshot {
    DevBuf<double> sites;     // (E)
    DevBuf<int32_t> chi;      // [T + 2]: chi, label_site
    DevBuf<DevScalars> sc;
    explicit operator bool() const { return sites != nullptr; }
    int copies(Ctx* c, bool restore);
    int save(Ctx* c) { return copies(c, false); }
    int restore(Ctx* c) { return copies(c, true); }
};

// The training workspace: everything ensure_workspace allocates or decides for (training set, options, capacity, element type).
// Buffers marked (E) hold elements of c->esz bytes behind their double* names.
struct TrainWs {
    // caches + workspaces (train set)
    DevBuf<double> LE, RE;    // (E)
    int64_t cache_elems = 0;
    DevBuf<double> bt, partial;      // (E)
    DevBuf<double> yhat, tile_loss, gradbuf, gram, lam, E, eig_ws, btn, norm_part;
    // four-launch chain (k_grad_s, k_gram_upd, k_eig_trivec, k_bond_tail): bt_new once more as [c][y][x] for the tail's contraction going
    // right; a tail whose on-device verification failed marks the sweep (DevScalars::redo) and the rest of it is redone on the six-launch chain
    DevBuf<double> btnT;
    // ... and what the side workgroups of k_eig_trivec leave for the tail (TailSide): [ntiles][TS_ST] dense S tiles, [ntiles][TS_P] overlap products
    DevBuf<double> tail_St, tail_P;
    // diagnostics: (start, end) stamps of every workgroup of the stamped k_bond_tail launch, [2 * TS_SPAN]; behind them the same of the side workgroups
    DevBuf<unsigned long long> tail_span;
    bool chain4_ok = false;
    bool rebuild_side = false;    // tail_pre and not MPST_REBUILD_SIDE=0: with rebuild_caches the side workgroups rebuild the caches, a row per bond
    bool tail_pre = false;    // chain4_ok and not MPST_TAIL_PRE=0: side workgroups form the S tile and the overlap product, else the tail itself
    int tail_force_fail = -1, tail_launches = 0;      // test hook (MPST_TAIL_FORCE_REDO=n): the n-th tail launch of the workspace reports a failed verification
    // sliced bond GEMMs (k_yhat_s / k_grad_s): slice contributions to yhat, loss pieces, arrival tickets
    DevBuf<double> b2_ypart, b2_lossp;
    DevBuf<unsigned int> b2_tick;
    DevBuf<unsigned long long> b2_dbg;   // bring-up stamps of the sliced kernels (MPST_B2_DEBUG builds)
    int b2_ksplit = 0, b2_norm_parts = 0;
    bool b2 = false;            // the fused chain uses k_yhat_s + k_grad_s instead of k_bond_fused + k_fused_reduce
    DevBuf<double> loss_trace;  // track_cost: [2(T-1)][update_iters + 1]
    int n_norm_part = 0;
    bool fused = false;        // bond tensors <= MAX_DIM^2 and no rescale[1]: the 7-launch chain of mpst_fused.hip
    int64_t partial_elems = 0;
    DevBuf<DevScalars> sc;
    DevBuf<double> norm2;
    DevBuf<double> norm_scratch;    // 3*cap*cap doubles for k_norm2 when they exceed its LDS
    // element-typed context
    DevBuf<double> tnorm_scratch;   // typed normalize: three complex cap x cap matrices
    DevBuf<int32_t> xLE, xRE, yexp; // typed: binary exponents of the environment rows / overlaps
    DevOwned<BigEig*, BigEig*, release_big> big;          // d*cap > MAX_DIM: library eigensolver at the capacity size (fallback of the blocked one)
    DevOwned<BlockedEig*, BlockedEig*, release_blocked> blk;    // d*cap > MAX_DIM: hand-written blocked eigensolver
    // large bonds, sweeps: the verdict of the blocked eigensolver is read once per sweep instead of once per bond (no host
    // synchronisation inside the sweep); a sweep in which any bond failed is redone from a snapshot, bond by bond
    bool big_opt = false;
    Snapshot snap;
    int big_force_fail = -1, big_solves = 0;          // test hook (MPST_BIG_FORCE_FAIL=n): the n-th solve of the workspace is marked failed
};

// The evaluation scratch, sized by the larger of the two data sets: replaced by ensure_eval
struct EvalWs {
    DevBuf<double> chainL[2], chainR[2];   // (E)
    DevBuf<int32_t> xchainL[2], xchainR[2];
    DevBuf<double> yeval, out3;
    DevBuf<int64_t> conf;
    DevBuf<int32_t> pred;
    int64_t eval_N = 0;
};

// What a context holds as the lead of a batch.  mpst_sweep_batch: the Views of the K fits on the device ([2][K]: plain, and the Gram
// launch's variant), the captured sweep and what it was captured for; mpst_classify_batch: the jobs and every fit's results in one block
struct BatchLead {
    DevBuf<View> batch_views;
    int batch_cap = 0;
    DevGraphExec batch_graph;
    std::vector<std::pair<uint64_t, uint64_t>> batch_key;   // (uid, epoch) per member: an address can be handed out again, a uid cannot
    DevBuf<uint8_t> score_buf;
    int64_t score_cap = 0;
};

struct Ctx {
    int device = 0;
    // session state, the context's lifetime.  Members are destroyed in reverse order: the stream outlives every event, buffer and graph.
    DevStream stream;
    DevEvent ev_start, ev_stop;
    std::vector<DevEvent> ev_pool;
    std::string err;
    mpst_options opt{};
    bool have_opt = false;
    int T = 0, d = 0, C = 0;
    // element type of the data sets and of the MPS (mpst_set_dataset's dtype = opts.dtype, RealRealHighDimension.jl:442).
    // typed: everything runs through the element-typed kernels of mpst_typed.hip (always for fp32 / complex; MPST_TYPED=1
    // sends Float64 through them too - the cross-check of the two implementations); the (E) buffers then hold
    // elements of esz bytes behind their double* names.
    int dtype = MPST_F64;
    bool have_dtype = false, typed = false;
    int zw = 1;               // 2: complex
    size_t esz = 8;           // bytes per element
    DataSet ds[2];
    bool have_mps = false;
    Mps mps;
    bool ws_ready = false;      // training workspace (caches, bond tensor, gradient, eigensolver) built for the current sizes
    TrainWs ws;
    bool eval_ready = false;    // evaluation scratch (chains, yeval, pred) built for max(N_train, N_test)
    EvalWs ev;
    BatchLead lead;
    bool caches_valid = false;  // LE / RE describe the current MPS: set by mpst_build_caches, cleared by whatever invalidates them
    int host_label_site = -1;   // host mirror of *label_site (set_mps, bond_step and sweep move it deterministically)
    // four-launch chain: which bond's overlaps the last tail launch left in b2_ypart (valid while nothing else touched the context:
    // bond_seq / epoch); held back while a marked sweep / bond is redone
    bool chain4_hold = false;
    int ynext_lid = -1;
    uint64_t ynext_epoch = 0, ynext_seq = 0, bond_seq = 0;
    int tail_redos = 0;
    int rebuild_steps = 0;      // rows rebuilt beside the eigensolver in the last sweep (DevScalars::rebuild_steps)
    int32_t ss_counts[2] = {0, 0};      // subspace eigensolver: bonds attempted / accepted, read where a sweep or a bond step synchronises anyway
    int64_t big_fallbacks = 0;        // bonds on which the blocked solver's verification asked for the library
    bool big_opt_active = false;
    int big_redos = 0;
    int big_cooldown = 0;             // sweeps left that read the verdict per bond after a sweep had to be redone
    // multi-GPU
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    // MPST_FORCE_COLLECTIVE=1 at mpst_comm_init: the sharded launch chain (loss in the message, all-reduce, norm pieces from the
    // summed gradient, plain stream) also with ONE rank - the RCCL leg then runs on every 1-GPU CI box (tests/test_gpu_multi.py)
    bool force_coll = false;
    // one-shot direct-write all-reduce (mpst_allreduce.hip): this rank's inbox (fine-grained device memory, exported
    // over IPC) and the peers' inboxes as mapped here (borrowed: ipc_release closes them)
    DevBuf<uint8_t> ipc_local;           // [2][nranks][slot] doubles | 16 flags | 2 counters
    void* ipc_peer[AR_MAX_RANKS] = {nullptr};
    int64_t ipc_slot = 0;
    size_t ipc_flag_off = 0, ipc_ctr_off = 0, ipc_bytes = 0;
    bool use_ipc = false;                // all peers attached: gradient and evaluation sums go through the one-shot path
    bool ipc_dead = false;               // a one-shot all-reduce timed out: its cross-rank state is undefined until the inboxes are exported again
    unsigned long long ar_epoch = 0;
    // profiling
    unsigned prof_mask = 0;
    struct Rec { int k; size_t e0, e1; };
    std::vector<Rec> recs;
    size_t ev_used = 0;
    double prof_us[16] = {0};
    double impute_phase_s[2] = {0, 0};   // last imputation call: environment pass, density sweep
    int impute_batched = 0;              // ... and whether its sweep ran sixteen instances per workgroup (k_imp_leftb)
    int impute_trig = 0;                 // ... and whether its densities were evaluated in closed form (Fourier states on a uniform grid)
    int impute_env_wgs = 0;              // ... the workgroups of its environment pass (one per instance with a missing site or not: the grid)
    int impute_chains = 0;               // ... and the chains (instance, trajectory) its sweep was launched for
    int64_t prof_cnt[16] = {0};
    // one full sweep captured as a hipGraph (bond dimensions live on the device and every grid is sized
    // for the capacity, so the launch sequence of a sweep never changes between sweeps); `epoch` is
    // bumped by every call that changes what the captured kernels were given
    DevGraphExec sweep_graph;
    uint64_t epoch = 1, graph_epoch = 0;
    int batch_hint = 1;            // mpst_set_batch_hint: this context will be advanced in batches of about that many fits
    uint64_t uid = 0;              // process-wide, never reused (mpst_create)
    ~Ctx();                        // the peers' inboxes are unmapped before the members go
};

int fail(Ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_err = buf;
    return code;
}

#define HIPC(c, call)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((c), MPST_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                   \
    } while (0)

template <typename T>
int dalloc(Ctx* c, DevBuf<T>& b, int64_t n) {
    b = DevBuf<T>();
    if (n <= 0) n = 1;
    hipError_t e = hipMalloc((void**)&b.h, (size_t)n * sizeof(T));
    if (e != hipSuccess) return fail(c, MPST_ERR_NOMEM, "hipMalloc of %lld bytes failed: %s", (long long)(n * sizeof(T)), hipGetErrorString(e));
    return 0;
}
// (E) buffers: `n` elements of c->esz bytes behind a double* name
int dalloc_e(Ctx* c, DevBuf<double>& b, int64_t n) {
    b = DevBuf<double>();         // what b held goes first: the peak is one buffer
    DevBuf<uint8_t> q;
    const int rc = dalloc(c, q, std::max<int64_t>(n, 1) * (int64_t)c->esz);
    b.h = (double*)q.h;
    q.h = nullptr;
    return rc;
}

View make_view(Ctx* c, int which) {
    View v{};
    const DataSet& s = c->ds[which];
    v.T = c->T; v.d = c->d; v.C = c->C; v.chi_max = c->opt.chi_max; v.cap = c->mps.cap;
    v.N = s.N;
    v.invN = s.Nglobal > 0 ? 1.0 / (double)s.Nglobal : 0.0;
    v.phi = s.phi; v.label = s.label; v.tiles = s.tiles; v.chunks = s.chunks;
    v.cls_chunk_off = s.cls_chunk_off; v.inv_count = s.inv_count;
    v.ntiles = s.ntiles; v.nchunks = s.nchunks;
    v.chi = c->mps.chi; v.label_site = c->mps.label_site; v.sites = c->mps.sites; v.site_stride = c->mps.site_stride;
    v.LE = c->ws.LE; v.RE = c->ws.RE; v.bt = c->ws.bt; v.yhat = c->ws.yhat; v.tile_loss = c->ws.tile_loss;
    v.ss_bt = c->ws.bt; v.ss_f32 = 0;
    v.partial = c->ws.partial; v.gradbuf = c->ws.gradbuf; v.gram = c->ws.gram; v.lam = c->ws.lam; v.E = c->ws.E; v.eig_ws = c->ws.eig_ws; v.sc = c->ws.sc;
    v.loss = c->opt.loss; v.optimiser = c->opt.optimiser; v.rescale_before = c->opt.rescale_before;
    v.rescale_after = c->opt.rescale_after; v.train_sep = c->opt.train_classes_separately; v.svd_alg = c->opt.svd_alg;
    v.eta = c->opt.eta; v.cutoff = c->opt.cutoff;
    const int pk = c->opt.loss == MPST_LOSS_MSE ? 1 : 0;
    v.parts = s.parts[pk]; v.part_off = s.part_off[pk]; v.nparts = s.nparts[pk];
    v.norm_part = c->ws.norm_part; v.n_norm_part = c->ws.n_norm_part; v.btn = c->ws.btn;
    v.btnT = (which == MPST_TRAIN && c->ws.chain4_ok && !c->chain4_hold) ? c->ws.btnT : nullptr;
    v.trace = nullptr; v.trace_it = 0; v.yhat_scaled = 0;
    v.cls_off = s.cls_off; v.ypart = c->ws.b2_ypart; v.lossp = c->ws.b2_lossp; v.tick = c->ws.b2_tick; v.b2_ksplit = c->ws.b2_ksplit; v.b2_nw = (c->batch_hint > 1 && c->d == 4) ? 4 : 8; v.dbg = c->ws.b2_dbg;
    {
        int32_t so = 0, to = 0;
        for (int k = 0; k <= MAX_C; ++k) {
            v.kcls_off[k] = so;
            v.kcls_tile[k] = to;
            if (k < (int)s.counts.size()) {
                so += (int32_t)s.counts[k];
                to += (int32_t)tiles_of(s.counts[k]);
            }
        }
    }
    return v;
}

TView make_tview(Ctx* c, int which) {
    TView t{};
    const DataSet& s = c->ds[which];
    t.T = c->T; t.d = c->d; t.C = c->C; t.chi_max = c->opt.chi_max; t.cap = c->mps.cap;
    t.cx = c->zw == 2; t.f32 = (c->dtype == MPST_F32 || c->dtype == MPST_C64);
    t.N = s.N;
    t.invN = s.Nglobal > 0 ? 1.0 / (double)s.Nglobal : 0.0;
    t.phi = s.phi; t.label = s.label; t.tiles = s.tiles; t.chunks = s.chunks; t.cls_chunk_off = s.cls_chunk_off; t.inv_count = s.inv_count;
    t.ntiles = s.ntiles; t.nchunks = s.nchunks;
    t.chi = c->mps.chi; t.label_site = c->mps.label_site; t.sites = c->mps.sites; t.site_stride = c->mps.site_stride;
    t.LE = c->ws.LE; t.RE = c->ws.RE; t.xLE = c->ws.xLE; t.xRE = c->ws.xRE; t.yexp = c->ws.yexp;
    t.bt = c->ws.bt; t.yhat = c->ws.yhat; t.tile_loss = c->ws.tile_loss; t.partial = c->ws.partial;
    t.gradbuf = c->ws.gradbuf; t.norm_part = c->ws.norm_part; t.n_norm_part = c->ws.n_norm_part;
    t.gram = c->ws.gram; t.E = c->ws.E; t.ldE = c->zw * c->mps.cap; t.sc = c->ws.sc;
    t.loss = c->opt.loss; t.optimiser = c->opt.optimiser; t.rescale_before = c->opt.rescale_before; t.rescale_after = c->opt.rescale_after;
    t.train_sep = c->opt.train_classes_separately;
    t.eta = c->opt.eta; t.cutoff = c->opt.cutoff;
    t.trace = nullptr; t.trace_it = 0; t.yhat_scaled = 0;
    return t;
}
// what the fp64 eigensolvers see of a typed context: the (embedded) Gram matrix, doubled counts for complex elements
View make_eig_view(Ctx* c) {
    View v{};
    v.T = c->T; v.d = c->d; v.C = c->C;
    v.chi_max = c->zw * c->opt.chi_max;
    v.cap = c->zw * c->mps.cap;
    v.chi = c->mps.chi; v.label_site = c->mps.label_site;
    v.gram = c->ws.gram; v.lam = c->ws.lam; v.E = c->ws.E; v.eig_ws = c->ws.eig_ws; v.sc = c->ws.sc;
    v.rescale_after = c->opt.rescale_after; v.svd_alg = c->opt.svd_alg; v.cutoff = c->opt.cutoff;
    v.zw = c->zw;
    v.ss_bt = c->ws.bt;                                             // the subspace eigensolver reads the bond tensor itself
    v.ss_f32 = (c->dtype == MPST_F32 || c->dtype == MPST_C64) ? 1 : 0;
    return v;
}

inline bool multi(const Ctx* c) { return c->nranks > 1 || c->force_coll; }

void ipc_release(struct Ctx* c);

// (re)allocate the evaluation scratch: sized by the larger of the two data sets, independent of the training
// workspace, so that (re)loading a TEST set never touches the environment caches
int ensure_eval(Ctx* c) {
    if (c->eval_ready) return 0;
    c->ev = EvalWs();
    EvalWs e;
    int rc;
    const int64_t en = std::max<int64_t>(1, std::max(c->ds[0].N, c->ds[1].N));
    e.eval_N = en;
    for (int k = 0; k < 2; ++k) {
        if ((rc = dalloc_e(c, e.chainL[k], en * c->mps.cap))) return rc;
        if ((rc = dalloc_e(c, e.chainR[k], en * c->mps.cap))) return rc;
        if (c->typed && ((rc = dalloc(c, e.xchainL[k], en)) || (rc = dalloc(c, e.xchainR[k], en)))) return rc;
    }
    if ((rc = dalloc(c, e.yeval, en * c->C * (c->typed ? 2 : 1)))) return rc;      // typed: (re, im) pairs
    if ((rc = dalloc(c, e.out3, 4))) return rc;
    if ((rc = dalloc(c, e.conf, (int64_t)MAX_C * MAX_C))) return rc;
    if ((rc = dalloc(c, e.pred, en))) return rc;
    c->ev = std::move(e);
    c->eval_ready = true;
    return 0;
}

// ---- the training workspace: one builder, parameterised by the element type (c->zw, c->esz) ---------------------------------
// The eigensolvers of bonds whose (embedded) Gram matrix of dimension n exceeds the LDS-resident solver.
int setup_big_eig(Ctx* c, TrainWs& w, int n, int ss_rows, int ss_cx) {
    int rc;
    if (n <= MAX_DIM) return 0;
    std::string e;
    if ((rc = big_eig_create(&w.big.h, n, c->stream, &e))) return fail(c, rc, "large-bond eigensolver: %s", e.c_str());
    const char* sel = getenv("MPST_BIG_EIG");
    if (!(sel && (strcmp(sel, "jacobi") == 0 || strcmp(sel, "rocsolver") == 0)) && (rc = blocked_eig_create(&w.blk.h, n, &e)))
        return fail(c, rc, "large-bond eigensolver: %s", e.c_str());
    // the randomised subspace solver in front of the exact one (complex Gram matrices arrive as embeddings)
    if (w.blk && (rc = blocked_eig_enable_subspace(w.blk, ss_rows, c->mps.cap, c->C, ss_cx, &e))) return fail(c, rc, "large-bond eigensolver: %s", e.c_str());
    // MPST_BIG_SYNC=1: read the eigensolver's verdict after every bond (one host synchronisation per bond) instead of once per sweep
    w.big_opt = w.blk && getenv("MPST_BIG_SYNC") == nullptr && getenv("MPST_BT_NO_COOP") == nullptr;
    if (const char* ff = getenv("MPST_BIG_FORCE_FAIL")) w.big_force_fail = atoi(ff);       // test hook: the n-th solve of the workspace is marked failed
    return 0;
}

// What only the element-typed context's workspace holds (mpst_typed.hip): its limits, the binary exponents of the environments,
// the shares of its gradient and norm kernels.  Everything that decides the truncation stays in fp64.
int workspace_typed(Ctx* c, TrainWs& w, int64_t Lmax) {
    const DataSet& tr = c->ds[MPST_TRAIN];
    const int dm = c->d * c->mps.cap, zw = c->zw;
    int rc;
    if (zw * dm > DIM_LIMIT || zw * c->mps.cap > CAP_LIMIT)
        return fail(c, MPST_ERR_UNSUPPORTED, "complex element type: 2*d*chi_max = %d (2*chi_max = %d) exceeds the eigensolver's limits %d, %d", zw * dm, zw * c->mps.cap, DIM_LIMIT, CAP_LIMIT);
    if (c->d > 32) return fail(c, MPST_ERR_UNSUPPORTED, "the element-typed sweep holds d <= 32");
    TView tv = make_tview(c, MPST_TRAIN);       // (its shape: the buffers are not there yet)
    if (typed_max_lds(tv) > 144 * 1024) return fail(c, MPST_ERR_UNSUPPORTED, "chi_max = %d, d = %d exceed the LDS staging of the element-typed kernels for this element type", c->mps.cap, c->d);
    if ((rc = dalloc(c, w.xLE, (int64_t)c->T * tr.N)) || (rc = dalloc(c, w.xRE, (int64_t)c->T * tr.N)) || (rc = dalloc(c, w.yexp, tr.N))) return rc;
    w.partial_elems = (int64_t)c->C * typed_grad_nsplit(tv, tr.nchunks) * Lmax;
    w.n_norm_part = typed_norm_parts(tv);
    if ((rc = dalloc(c, w.tnorm_scratch, (int64_t)6 * c->mps.cap * c->mps.cap))) return rc;
    return 0;
}

// What only the Float64 context's workspace holds: which launch chain its bonds run (fused, sliced pair, four launches) and the
// buffers of that chain.
int workspace_f64(Ctx* c, TrainWs& w, int64_t Lmax) {
    const DataSet& tr = c->ds[MPST_TRAIN];
    const int dm = c->d * c->mps.cap;
    int rc;
    w.fused = dm <= MAX_DIM && !c->opt.rescale_before && getenv("MPST_NO_FUSED") == nullptr;
    // Which pair forms the gradient on the fused chain.  The sliced kernels (k_yhat_s + k_grad_s) move tens of KB per workgroup
    // and no partial gradients: 26 us against 31 us per bond at N = 4096, 11.6 MB against 40 MB of HBM traffic.  Their cost per
    // series is higher though (every series is read by 8 slice- and 16 block-workgroups: 2.7 against 1.5 us per 1000 series),
    // so from about 8000 series per rank the persistent k_bond_fused + k_fused_reduce pair wins (N = 32768: 75 against 105 us;
    // profiles/r03_*).  MPST_B2=0 / 1 forces either.
    {
        const char* e = getenv("MPST_B2");
        const bool want = e ? atoi(e) != 0 : (tr.N <= 8192 && getenv("MPST_NO_B2") == nullptr);
        w.b2 = w.fused && c->d >= 2 && c->d <= 16 && want;
    }
    if (w.fused) {
        w.partial_elems = (int64_t)std::max(tr.nparts[0], tr.nparts[1]) * Lmax;   // independent of N: one partial per persistent workgroup
        if (w.b2) {
            View gv{};
            gv.C = c->C; gv.d = c->d; gv.cap = c->mps.cap;
            const int64_t max_pass = tr.N;                  // MSE walks every series in every pass; KLD at most that
            w.b2_ksplit = b2_ksplit(gv, max_pass);
            // a context that runs in batches of K fits shares the chip with K - 1 others: fewer, longer shares per gradient block
            // (less hand-over per fit; the share count fixes the order of the partial sums, so it belongs to the context, not to the call)
            // (d = 4: the batched launches run k_grad_s with four waves per workgroup, two workgroups per CU - twice the workgroups fill the chip)
            if (c->batch_hint > 1 && getenv("MPST_B2_KSPLIT") == nullptr)
                w.b2_ksplit = c->d == 4 ? std::max(1, std::min(w.b2_ksplit, 2 * w.b2_ksplit / std::min(c->batch_hint, 16)))
                                        : std::max(1, w.b2_ksplit / std::min(c->batch_hint, 8));
            w.b2_norm_parts = c->C * b2_blocks_cap(gv);
            w.partial_elems = std::max(w.partial_elems, b2_partial_elems(gv, max_pass));
            if ((rc = dalloc(c, w.b2_ypart, (int64_t)8 * c->C * tr.N))) return rc;
            if ((rc = dalloc(c, w.b2_lossp, (int64_t)c->C * 64))) return rc;     // GS_MAXKS shares per class
            if ((rc = dalloc(c, w.b2_tick, (int64_t)w.b2_norm_parts + 1))) return rc;
            HIPC(c, hipMemset(w.b2_tick, 0, (size_t)(w.b2_norm_parts + 1) * sizeof(unsigned int)));
#ifdef MPST_B2_DEBUG
            if ((rc = dalloc(c, w.b2_dbg, 8192 * 8))) return rc;
            HIPC(c, hipMemset(w.b2_dbg, 0, 8192 * 8 * sizeof(unsigned long long)));
#endif
        }
    } else {
        const int nbcap = ((dm + GB - 1) / GB) * ((dm + GB - 1) / GB);
        w.partial_elems = (int64_t)c->C * grad_nsplit(tr.nchunks, nbcap, c->C) * Lmax;    // one partial per k_grad workgroup share, independent of N
    }
    if ((rc = dalloc(c, w.btn, c->C * Lmax))) return rc;
    {
        const char* e4 = getenv("MPST_CHAIN4");
        // (a context that is advanced in batches keeps the six-launch chain mpst_sweep_batch runs: its solo and its batched sweeps agree bit for bit)
        w.chain4_ok = w.fused && w.b2 && c->batch_hint <= 1 && !(e4 && e4[0] == '0');
        if (const char* ff = getenv("MPST_TAIL_FORCE_REDO")) w.tail_force_fail = atoi(ff);
        const char* ep = getenv("MPST_TAIL_PRE");
        w.tail_pre = w.chain4_ok && !(ep && ep[0] == '0');
        const char* er = getenv("MPST_REBUILD_SIDE");
        w.rebuild_side = w.tail_pre && !(er && er[0] == '0');
        if (w.chain4_ok && (rc = dalloc(c, w.btnT, c->C * Lmax))) return rc;
        if (w.tail_pre && (rc = dalloc(c, w.tail_St, (int64_t)tr.ntiles * TS_ST))) return rc;
        if (w.tail_pre && (rc = dalloc(c, w.tail_P, (int64_t)tr.ntiles * TS_P))) return rc;
        if (w.chain4_ok && (rc = dalloc(c, w.tail_span, 4 * TS_SPAN))) return rc;
        if (w.chain4_ok) HIPC(c, hipMemset(w.tail_span, 0, 4 * TS_SPAN * sizeof(unsigned long long)));
    }
    w.n_norm_part = (int)((c->C * Lmax + 63) / 64);      // RED_E entries per workgroup of k_fused_reduce
    if ((rc = dalloc(c, w.norm_scratch, (int64_t)3 * c->mps.cap * c->mps.cap))) return rc;
    return 0;
}

// everything whose size depends on (training set, options, capacity).  (E) buffers hold elements of c->esz bytes;
// the Gram matrix, its spectrum and the gradient message are fp64 in every element type (zw doubles per complex entry).
int build_workspace(Ctx* c, TrainWs& w) {
    const DataSet& tr = c->ds[MPST_TRAIN];
    const int dm = c->d * c->mps.cap, zw = c->zw;
    const int64_t Lmax = (int64_t)dm * dm;
    int rc;
    w.cache_elems = (int64_t)c->T * tr.N * c->mps.cap;
    if ((rc = c->typed ? workspace_typed(c, w, Lmax) : workspace_f64(c, w, Lmax))) return rc;
    if ((rc = dalloc_e(c, w.LE, w.cache_elems))) return rc;
    if ((rc = dalloc_e(c, w.RE, w.cache_elems))) return rc;
    if ((rc = dalloc_e(c, w.bt, c->C * Lmax))) return rc;
    if ((rc = dalloc(c, w.yhat, (int64_t)(c->typed ? 2 : 1) * c->C * tr.N))) return rc;      // typed: (re, im) pairs
    if ((rc = dalloc(c, w.tile_loss, std::max<int64_t>((int64_t)c->C * tr.ntiles, c->typed ? 1 : std::max(tr.nparts[0], tr.nparts[1]))))) return rc;
    if ((rc = dalloc_e(c, w.partial, w.partial_elems))) return rc;
    if ((rc = dalloc(c, w.norm_part, c->typed ? w.n_norm_part : std::max(w.n_norm_part, w.b2_norm_parts)))) return rc;
    if ((rc = dalloc(c, w.loss_trace, (int64_t)2 * (c->T - 1) * (c->opt.update_iters + 1)))) return rc;
    HIPC(c, hipMemset(w.loss_trace, 0, (size_t)2 * (c->T - 1) * (c->opt.update_iters + 1) * sizeof(double)));
    if ((rc = dalloc(c, w.gradbuf, 2 + c->C * Lmax * zw))) return rc;
    HIPC(c, hipMemset(w.gradbuf, 0, (size_t)(2 + c->C * Lmax * zw) * sizeof(double)));
    const int ne = std::max(zw * dm, MAX_DIM);
    if ((rc = dalloc(c, w.gram, (int64_t)ne * ne))) return rc;
    if ((rc = dalloc(c, w.lam, ne + 2))) return rc;
    if ((rc = dalloc(c, w.E, (int64_t)ne * zw * c->mps.cap))) return rc;
    if ((rc = setup_big_eig(c, w, zw * dm, zw * c->C * dm, zw == 2))) return rc;
    if ((rc = dalloc(c, w.eig_ws, (int64_t)eig_workspace_doubles()))) return rc;
    HIPC(c, hipMemset(w.eig_ws, 0, eig_workspace_doubles() * sizeof(double)));
    if ((rc = dalloc(c, w.sc, 1))) return rc;
    HIPC(c, hipMemset(w.sc, 0, sizeof(DevScalars)));
    return dalloc(c, w.norm2, 1);
}

// The old workspace goes first (the caches alone reach gigabytes), the new one is built aside in `w` and moved in complete: a
// failure on the way leaves the context without a workspace (ws_ready false), never with half of one beside half of another.
int ensure_workspace(Ctx* c) {
    if (!c->have_opt) return fail(c, MPST_ERR_INVALID, "mpst_set_options must be called first");
    if (!c->have_mps) return fail(c, MPST_ERR_INVALID, "mpst_set_mps must be called first");
    if (c->ws_ready) return ensure_eval(c);
    const DataSet& tr = c->ds[MPST_TRAIN];
    if (tr.N <= 0) return fail(c, MPST_ERR_INVALID, "no training data set (mpst_set_dataset)");
    const int dm = c->d * c->mps.cap;
    if (dm > DIM_LIMIT || c->mps.cap > CAP_LIMIT)
        return fail(c, MPST_ERR_UNSUPPORTED, "d*chi_max = %d (chi_max = %d) exceeds the engine's limits d*chi_max <= %d, chi_max <= %d", dm, c->mps.cap, DIM_LIMIT, CAP_LIMIT);
    if (c->C > MAX_C) return fail(c, MPST_ERR_UNSUPPORTED, "more than %d classes unsupported", MAX_C);
    if (c->ipc_local && 2 + (int64_t)c->C * dm * dm * c->zw > c->ipc_slot) ipc_release(c);   // inbox slots too small for the new capacity: export again
    c->caches_valid = false;
    c->ynext_lid = -1;
    c->ws = TrainWs();
    TrainWs w;
    if (int rc = build_workspace(c, w)) return rc;
    hipError_t ea = init_kernel_attrs(c->device);
    if (ea == hipSuccess) ea = eig_init_attrs(c->device);
    if (ea == hipSuccess) ea = c->typed ? typed_init_attrs(c->device) : b2_init_attrs(c->device);
    if (ea != hipSuccess) return fail(c, MPST_ERR_DEVICE, "hipFuncSetAttribute failed: %s", hipGetErrorString(ea));
    c->ws = std::move(w);
    c->ws_ready = true;
    c->eval_ready = false;
    c->epoch++;
    return ensure_eval(c);
}

// clears the sticky error flag and the per-sweep diagnostics (status, eig_sweeps_total, eig_fallbacks are adjacent);
// enqueued at the head of every sweep / bond step - inside the captured graph too - so that a context recovers
// after a failed decomposition (the class of failure tune() retries on)
// The subspace eigensolver's counters, read where the stream has just been synchronised (after a sweep, a bond step, a batch): the info
// query returns these and never touches the stream.
static void refresh_ss_counts(Ctx* c) {
    if (c->ws.blk) (void)blocked_eig_subspace_counts(c->ws.blk, c->stream, &c->ss_counts[0], &c->ss_counts[1]);
}
int enqueue_reset_status(Ctx* c) {
    static_assert(offsetof(DevScalars, eig_fallbacks) == offsetof(DevScalars, status) + 8, "status / eig_sweeps_total / eig_fallbacks adjacent");
    HIPC(c, hipMemsetAsync(&c->ws.sc.h->status, 0, 12, c->stream));
    static_assert(offsetof(DevScalars, rebuild_steps) == offsetof(DevScalars, redo) + 4, "redo / rebuild_steps adjacent");
    HIPC(c, hipMemsetAsync(&c->ws.sc.h->redo, 0, 8, c->stream));
    return 0;
}

// ---- profiling helpers: HIP events on the stream the kernels are launched on -------------
hipEvent_t pool_event(Ctx* c) {
    if (c->ev_used == c->ev_pool.size()) {
        c->ev_pool.emplace_back();
        (void)hipEventCreate(&c->ev_pool.back().h);
    }
    return c->ev_pool[c->ev_used++];
}
struct ProfScope {
    Ctx* c; int k; bool on; size_t e0 = 0;
    ProfScope(Ctx* c_, int k_) : c(c_), k(k_), on((c_->prof_mask >> k_) & 1u) {
        if (on) { e0 = c->ev_used; (void)hipEventRecord(pool_event(c), c->stream); }
    }
    ~ProfScope() {
        if (on) { size_t e1 = c->ev_used; (void)hipEventRecord(pool_event(c), c->stream); c->recs.push_back({k, e0, e1}); }
    }
};
void prof_collect(Ctx* c) {
    for (auto& r : c->recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_pool[r.e0], c->ev_pool[r.e1]) == hipSuccess) {
            c->prof_us[r.k] += 1e3 * ms;
            c->prof_cnt[r.k] += 1;
        }
    }
    c->recs.clear();
    c->ev_used = 0;
}

// ---- sum over ranks of a device buffer: the one-shot path when the inboxes are attached, else RCCL ---------------
void ipc_release(struct Ctx* c) {
    for (int r = 0; r < AR_MAX_RANKS; ++r) {
        if (c->ipc_peer[r] && c->ipc_peer[r] != c->ipc_local.h) (void)hipIpcCloseMemHandle(c->ipc_peer[r]);
        c->ipc_peer[r] = nullptr;
    }
    c->ipc_local = DevBuf<uint8_t>();
    c->use_ipc = false;
}
Ctx::~Ctx() { ipc_release(this); }
int enqueue_allreduce(Ctx* c, double* buf, int64_t n_fixed, int lid) {
    if (!multi(c)) return 0;
    if (c->use_ipc) {
        ArParams p{};
        for (int r = 0; r < c->nranks; ++r) {
            p.inbox[r] = (double*)c->ipc_peer[r];
            p.flags[r] = (unsigned long long*)((char*)c->ipc_peer[r] + c->ipc_flag_off);
        }
        p.buf = buf;
        p.status = &c->ws.sc.h->status;
        p.dbg = c->ws.sc.h->pad;
        p.counter = (unsigned int*)((char*)c->ipc_local.h + c->ipc_ctr_off);
        p.nranks = c->nranks; p.rank = c->rank; p.slot = c->ipc_slot;
        p.epoch = ++c->ar_epoch;
        {
            static const double secs = [] { const char* e = getenv("MPST_AR_TIMEOUT_S"); const double v = e ? atof(e) : 10.0; return v > 0.0 ? v : 10.0; }();
            p.spin_limit = (long long)(secs * 2.4e9);
        }
        p.chi = c->mps.chi; p.lid = lid; p.C = c->C * c->zw; p.d = c->d; p.n_fixed = n_fixed;      // complex gradients: (re, im) pairs
        if (lid < 0 && n_fixed > c->ipc_slot) return fail(c, MPST_ERR_INVALID, "all-reduce message exceeds the inbox slot");
        launch_allreduce_oneshot(p, c->stream);
        return 0;
    }
    if (c->ipc_dead && !c->comm)
        return fail(c, MPST_ERR_DEVICE, "the one-shot all-reduce timed out earlier: export and attach the inboxes again (mpst_comm_ipc_export / _attach)");
    if (!c->comm) return fail(c, MPST_ERR_INVALID, "%d ranks but neither an RCCL communicator nor attached inboxes", c->nranks);
    const size_t cnt = lid >= 0 ? 2 + (size_t)c->zw * c->C * c->d * c->mps.cap * c->d * c->mps.cap : (size_t)n_fixed;
    Rccl* nc = rccl_ready(nullptr);
    if (!nc) return fail(c, MPST_ERR_DEVICE, "RCCL is not available");
    ncclResult_t r = nc->AllReduce(buf, buf, cnt, ncclDouble, ncclSum, c->comm, c->stream);
    if (r != ncclSuccess) return fail(c, MPST_ERR_DEVICE, "ncclAllReduce: %s", nc->GetErrorString(r));
    return 0;
}

// ---- eigensolver of a bond whose Gram matrix exceeds the LDS-resident solver (both element paths) -----------------------
int enqueue_big_eig(Ctx* c, const View& v, int lid, int going_left) {
    hipStream_t s = c->stream;
    int need_lib = 1;
    if (c->ws.blk && c->big_opt_active) {
        if (launch_eig_blocked_nosync(v, lid, going_left, c->ws.blk, s)) return fail(c, MPST_ERR_DEVICE, "blocked eigensolver failed at bond %d: %s", lid, hipGetErrorString(hipGetLastError()));
        if (c->ws.big_force_fail >= 0 && c->ws.big_solves++ == c->ws.big_force_fail) blocked_eig_force_sticky(c->ws.blk, s);      // test hook
        need_lib = 0;
    } else if (c->ws.blk) {
        need_lib = launch_eig_blocked(v, lid, going_left, nullptr, 0, nullptr, nullptr, nullptr, c->ws.blk, s);
        if (need_lib < 0) return fail(c, MPST_ERR_DEVICE, "blocked eigensolver failed at bond %d: %s", lid, hipGetErrorString(hipGetLastError()));
        if (need_lib) c->big_fallbacks++;
    }
    if (need_lib && launch_eig_big(v, lid, going_left, c->ws.big, s)) return fail(c, MPST_ERR_DEVICE, "the large-bond Jacobi fallback could not be launched at bond %d", lid);
    return 0;
}
// the eigensolver of bond lid on the Gram matrix of v: the large-bond route, or stage 0 (tri, or tri + vec merged), 1 (vec), 2 (fin)
int enqueue_eig(Ctx* c, const View& v, int lid, int going_left) {
    if (c->ws.big) {
        ProfScope p(c, K_EIG_TRI);
        return enqueue_big_eig(c, v, lid, going_left);
    }
    { ProfScope p(c, K_EIG_TRI); launch_eig(v, lid, going_left, 0, c->stream); }
    if (!eig_merged()) { ProfScope p(c, K_EIG_VEC); launch_eig(v, lid, going_left, 1, c->stream); }
    { ProfScope p(c, K_EIG_FIN); launch_eig(v, lid, going_left, 2, c->stream); }
    return 0;
}
// one environment step (mpst_bond_plan.h) as a launch: k_tenv (the site tensor is the map, the rows' exponents alongside) or k_env
void launch_tenv_step(Ctx* c, const TView& t, const EnvStep& e) {
    const int64_t cs = (int64_t)t.N * t.cap;
    double* rows = e.left_side ? c->ws.LE : c->ws.RE;
    int32_t* x = e.left_side ? c->ws.xLE : c->ws.xRE;
    launch_tenv(t, e.site, e.left_side, env_row_e(rows, e.prev_site, cs, c->esz), env_row(x, e.prev_site, t.N), e.prev_bond,
                e.left_side ? ENV_M_SITE : ENV_M_SITE_T, e.out_bond, env_row_e(rows, e.out_site, cs, c->esz), env_row(x, e.out_site, t.N), c->stream);
}
void launch_env_step(Ctx* c, const View& v, const EnvStep& e, int mode, int bt_lid = -1) {
    const int64_t cs = (int64_t)v.N * v.cap;
    double* rows = e.left_side ? v.LE : v.RE;
    launch_env(v, e.site, e.left_side, env_row(rows, e.prev_site, cs), e.prev_bond, mode, e.out_bond, env_row(rows, e.out_site, cs), c->stream, bt_lid);
}

// ---- the per-bond chain of the element-typed sweep (mpst_typed.hip) -----------------------------------------------------
int enqueue_bond_typed(Ctx* c, int lid, int going_left, int trace_row) {
    hipStream_t s = c->stream;
    TView t = make_tview(c, MPST_TRAIN);
    const int n_it = c->opt.update_iters;
    if (c->opt.track_cost && trace_row >= 0) t.trace = c->ws.loss_trace + (int64_t)trace_row * (n_it + 1);
    { ProfScope p(c, K_BT); launch_tbt_assemble(t, lid, s); }                    // flatten_bt
    if (t.rescale_before) launch_tbt_prescale(t, lid, s);
    for (int it = 0; it < n_it; ++it) {
        { ProfScope p(c, K_YHAT); launch_tyhat(t, lid, s); }
        { ProfScope p(c, K_GRAD); launch_tgrad(t, lid, s); }
        { ProfScope p(c, K_UPDATE); launch_tgrad_reduce(t, lid, s); }
        if (multi(c)) {
            ProfScope p(c, K_ALLREDUCE);
            int rc = enqueue_allreduce(c, c->ws.gradbuf, 0, lid);
            if (rc) return rc;
            launch_tgrad_norm(t, lid, s);
        }
        t.trace_it = it;
        { ProfScope p(c, K_UPDATE); launch_tupdate(t, lid, it == 0, s); }
    }
    { ProfScope p(c, K_GRAM); launch_tgram(t, lid, going_left, s); }             // decomposeBT: Gram matrix, fp64
    if (int rc = enqueue_eig(c, make_eig_view(c), lid, going_left)) return rc;
    if (t.trace) {          // track_cost: the loss at the updated (and, with rescale[2], normalised) bond tensor
        TView ty = t;
        ty.yhat_scaled = t.rescale_after;
        launch_tyhat(ty, lid, s);
        View vt = make_view(c, MPST_TRAIN);
        vt.trace = t.trace;
        vt.trace_it = n_it;
        launch_trace_loss(vt, s);
        if (multi(c)) {
            int rc = enqueue_allreduce(c, vt.trace + n_it, 1, -1);
            if (rc) return rc;
        }
    }
    { ProfScope p(c, K_SPLIT); launch_tsplit(t, lid, going_left, s); }
    { ProfScope p(c, K_ENV); launch_tenv_step(c, t, env_step_of_bond(lid, going_left, c->T)); }     // update_caches!: the new site tensor is the map
    return 0;
}
// construct_caches of the typed context: left environments of sites [0, upto), right environments of sites (from, T-1]
void enqueue_caches_typed(Ctx* c, int left_upto, int right_from) {
    TView t = make_tview(c, MPST_TRAIN);
    ProfScope p(c, K_ENV);
    for (int j = 0; j < left_upto && j <= c->T - 2; ++j) launch_tenv_step(c, t, env_step(j, 1, c->T));
    for (int j = c->T - 1; j > right_from && j >= 1; --j) launch_tenv_step(c, t, env_step(j, 0, c->T));
}

// ---- the chain decisions, each taken and reported (mpst_get_info) through one predicate ------------------------------------
// The 2(T-1) x 11 launches of a sweep are replayed from a hipGraph: nothing in the sequence depends
// on host-side state (bond dimensions are read on the device), and the pre-built dispatch packets
// shorten the dependent kernel-to-kernel hand-over that dominates the small kernels.  Per-kernel
// profiling and the RCCL leg keep the plain stream path.
// (large bonds stay on the plain stream: replaying their ~8000 launches from a graph was measured to gain nothing - 725.0
// against 724.5 ms per sweep at (8192, 200, 64, 8) - and a capture must not overlap other threads' legacy-stream copies)
bool sweep_uses_graph(const Ctx* c) { return !multi(c) && !c->ws.big && c->prof_mask == 0 && getenv("MPST_NO_GRAPH") == nullptr; }
// four launches per bond: k_eig_fin, k_env_split and the NEXT bond's k_yhat_s in one (k_bond_tail, mpst_fused.hip)
bool bond_uses_tail(const Ctx* c, const View& v, bool traced) {
    return c->ws.chain4_ok && !c->chain4_hold && c->ws.b2 && !multi(c) && c->opt.update_iters == 1 && !traced && eig_merged() && bond_tail_supported(v);
}
// the context can join a batch (mpst_sweep_batch): the headline chain, six launches per bond
bool batchable(const Ctx* c) {
    return c->ws.fused && c->ws.b2 && !c->typed && !multi(c) && eig_merged() && c->opt.update_iters == 1 && !c->opt.track_cost && !c->opt.rebuild_caches &&
           c->prof_mask == 0;
}
// the four-launch chain held back while a marked sweep / bond is redone on the six-launch chain: views made meanwhile carry no btnT
struct Chain4Hold {
    bool& h;
    explicit Chain4Hold(Ctx* c) : h(c->chain4_hold) { h = true; }
    ~Chain4Hold() { h = false; }
};

// ---- the per-bond launch chain (RealRealHighDimension.jl:733-762 / :777-801) ---------------
// have_bt: the bond tensor of this bond was already assembled by the previous bond's environment
// kernel; b.next_lid >= 0: assemble that bond's tensor inside this bond's environment kernel.
// rebuild_side: the bond's eigensolver launch carries a rebuild job (rebuild_side_on)
int enqueue_bond(Ctx* c, const View& v_in, const BondSlot& b, bool have_bt = false, int trace_row = -1, bool rebuild_side = false) {
    const int lid = b.lid, going_left = b.going_left, next_bt_lid = b.next_lid;
    if (c->typed) return enqueue_bond_typed(c, lid, going_left, trace_row);
    hipStream_t s = c->stream;
    View v = v_in;
    const int n_it = c->opt.update_iters;
    if (c->opt.track_cost && trace_row >= 0) v.trace = c->ws.loss_trace + (int64_t)trace_row * (n_it + 1);
    // track_cost: the loss at the updated (and, with rescale[2], normalised) bond tensor - one more forward pass over the batch
    auto trace_final = [&](const double* bt_new) -> int {
        if (!v.trace) return 0;
        View vy = v;
        vy.bt = const_cast<double*>(bt_new);
        vy.yhat_scaled = v.rescale_after;
        vy.trace_it = n_it;
        launch_yhat(vy, lid, s);
        launch_trace_loss(vy, s);
        // a shard's tile losses carry the GLOBAL 1/N: the sum over the ranks is the loss the single-rank run records
        if (multi(c)) return enqueue_allreduce(c, vy.trace + n_it, 1, -1);
        return 0;
    };
    const uint64_t seq_before = c->bond_seq++;
    if (c->ws.fused) {
        const int iters = c->opt.update_iters;
        // the next bond's tensor is assembled by this bond's last launch when the sweep moves on in the same direction
        const int chain = b.chains_into_next ? 1 : 0;
        const bool use4 = bond_uses_tail(c, v, v.trace != nullptr);
        // ... whose overlaps are this bond's if the launch before this one was the neighbouring bond's tail
        const bool y_ready = use4 && c->ynext_lid == lid && c->ynext_epoch == c->epoch && c->ynext_seq == seq_before;
        c->ynext_lid = -1;
        if (!have_bt) { ProfScope p(c, K_BT); launch_bt_assemble(v, lid, s); }   // flatten_bt :733/:777
        View vl = v;                      // after k_grad_s on one rank the loss is still in pieces (bond_loss)
        vl.n_lossp = c->ws.b2 ? c->ws.b2_ksplit : 0;
        for (int it = 0; it < iters; ++it) {                                     // TSGO/custGD :44,:75
            if (c->ws.b2) {
                if (!(y_ready && it == 0)) { ProfScope p(c, K_YHAT); launch_yhat_s(v, lid, s); }           // yhat, by column slices of B_c
                { ProfScope p(c, K_GRAD); launch_grad_s(v, lid, s); }           // gradient blocks, reduced by their last arriver
                if (multi(c)) launch_loss_sum(vl, s);                      // the loss travels in gradbuf[0]
            } else {
                { ProfScope p(c, K_GRAD); launch_bond_fused(v, lid, 0, s); }    // yhat + gradient partials
                { ProfScope p(c, K_UPDATE); launch_fused_reduce(v, lid, s); }
            }
            if (multi(c)) {
                ProfScope p(c, K_ALLREDUCE);
                int rc = enqueue_allreduce(c, c->ws.gradbuf, 0, lid);
                if (rc) return rc;
                launch_grad_norm(v, lid, s);
            }
            v.trace_it = it;
            if (it + 1 < iters) {
                ProfScope p(c, K_UPDATE);
                View vu = v;
                if (c->ws.b2 && !multi(c)) vu.n_lossp = c->ws.b2_ksplit;
                launch_update(vu, lid, it == 0, s);
            }
        }
        {
            ProfScope p(c, K_GRAM);                                               // last step + decomposeBT :756/:798
            View vg = v;
            if (c->ws.b2 && !multi(c)) vg.n_lossp = c->ws.b2_ksplit;
            // pieces of ||grad||^2: one per gradient block from k_grad_s; after an all-reduce k_grad_norm has rewritten them
            if (c->ws.b2 && !multi(c)) vg.n_norm_part = c->ws.b2_norm_parts;
            if (!use4) vg.btnT = nullptr;
            launch_gram_upd(vg, lid, going_left, iters == 1, s);
        }
        if (use4) {
            const int nxt = going_left ? lid - 1 : lid + 1;
            const int want = (nxt >= 0 && nxt <= c->T - 2) ? 1 : 0;
            // what of the tail needs no eigenvector rides in the eigensolver's launch, on the CUs it leaves empty (TailSide)
            TailSide sd{};
            const TailSide* pre = c->ws.tail_pre ? &sd : nullptr;
            if (pre) {
                tail_side_operands(v, lid, going_left, sd);
                sd.St = c->ws.tail_St;
                sd.P = c->ws.tail_P;
                sd.span = tail_stamped(v, lid, going_left) ? c->ws.tail_span + 2 * TS_SPAN : nullptr;
                sd.want_next = want;
                if (rebuild_side) tail_side_rebuild_job(v, lid, going_left, sd);
            }
            { ProfScope p(c, K_EIG_TRI); launch_eig(v, lid, going_left, 0, s, pre); }
            ProfScope p(c, K_ENV);                                                // verification, back-split, update_caches!, next yhat
            launch_bond_tail(v, lid, going_left, chain, want | (c->ws.tail_launches++ == c->ws.tail_force_fail ? 4 : 0), c->ws.tail_span, pre, s);
            if (want) {
                c->ynext_lid = nxt;
                c->ynext_epoch = c->epoch;
                c->ynext_seq = c->bond_seq;
            }
            return 0;
        }
        if (int rc = enqueue_eig(c, v, lid, going_left)) return rc;
        { int rc = trace_final(c->ws.btn); if (rc) return rc; }
        { ProfScope p(c, K_ENV); launch_env_split(v, lid, going_left, chain, s); }      // back-split + update_caches! :759/:799
        return 0;
    }
    if (!have_bt) { ProfScope p(c, K_BT); launch_bt_assemble(v, lid, s); }      // flatten_bt :733/:777
    if (v.rescale_before) launch_bt_prescale(v, lid, s);                        // loss_functions.jl:109
    for (int it = 0; it < c->opt.update_iters; ++it) {                          // TSGO/custGD :44,:75
        { ProfScope p(c, K_YHAT); launch_yhat(v, lid, s); }
        { ProfScope p(c, K_GRAD); launch_grad(v, lid, s); }
        { ProfScope p(c, K_UPDATE); launch_grad_reduce(v, lid, s); }
        if (multi(c)) {
            ProfScope p(c, K_ALLREDUCE);
            int rc = enqueue_allreduce(c, c->ws.gradbuf, 0, lid);
            if (rc) return rc;
        }
        v.trace_it = it;
        { ProfScope p(c, K_UPDATE); launch_update(v, lid, it == 0, s); }
    }
    { ProfScope p(c, K_GRAM); launch_gram(v, lid, going_left, s); }            // decomposeBT :756/:798
    if (int rc = enqueue_eig(c, v, lid, going_left)) return rc;
    { int rc = trace_final(c->ws.bt); if (rc) return rc; }
    { ProfScope p(c, K_SPLIT); launch_split(v, lid, going_left, s); }
    { ProfScope p(c, K_ENV); launch_env_step(c, v, env_step_of_bond(lid, going_left, c->T), ENV_M_E, next_bt_lid); }      // update_caches! :759/:799
    return 0;
}

// MPST_ENV_WALK=0: construct_caches as one k_env launch per site (the same bits)
bool env_walk_on(const Ctx* c, const View& v) {
    const char* e = getenv("MPST_ENV_WALK");
    return !c->typed && !(e && e[0] == '0') && env_walk_supported(v);
}

// The two construct_caches of a sweep (rebuild_caches) hidden beside the eigensolver: every bond's k_eig_trivec launch rebuilds one row
// on its side workgroups (TailSide::rb_site) and a closing walk of two steps per half-sweep does the rest.  Only where a bond runs the
// four-launch chain with side workgroups and a walk could do the rebuild; MPST_REBUILD_SIDE=0: the full walks.  Profiling sweeps keep
// the full walks (their per-kernel times are those of the launches they name).
bool rebuild_side_on(const Ctx* c, const View& v) {
    return c->opt.rebuild_caches && c->ws.rebuild_side && c->ws.tail_pre && c->prof_mask == 0 && bond_uses_tail(c, v, c->opt.track_cost != 0) &&
           env_walk_on(c, v);
}

// construct_caches (RealRealHighDimension.jl:45-103) around the label site ls: LE[0 .. ls-1] and RE[T-1 .. ls+1].  ls = T - 1 is
// construct_caches(W; going_left=true), ls = 0 going_left=false.  One launch per side where every workgroup can walk the chain with
// its 16 series (k_env_walk: the bits of the per-site launches; a side without sites launches nothing), else one per site.
// first > 0: the rows of the first `first` steps of each side exist already (the side workgroups rebuilt them): the walks start there.
void enqueue_caches(Ctx* c, const View& v, int ls, int first = 0) {
    if (c->typed) return enqueue_caches_typed(c, ls, ls);
    ProfScope p(c, K_ENV);
    if (env_walk_on(c, v)) {
        launch_env_walk(v, 1, std::min(ls, c->T - 1), c->stream, first);
        launch_env_walk(v, 0, c->T - 1 - ls, c->stream, first);
        return;
    }
    for (int j = 0; j < ls && j <= c->T - 2; ++j) launch_env_step(c, v, env_step(j, 1, c->T), ENV_M_SITE);
    for (int j = c->T - 1; j > ls && j >= 1; --j) launch_env_step(c, v, env_step(j, 0, c->T), ENV_M_SITE_T);
}

// ---- a sweep as a hipGraph, and what it left ----------------------------------------------------------------------------------
// What `enqueue` puts on the stream, captured (thread-local: other threads' work is none of this capture's) and instantiated into
// exec, whose previous graph goes first.  `enqueue` returns 0 or an error it has reported itself; a capture that does not end in a
// graph is reported with `end_text` and the end of capture's error.
using DevGraph = DevOwned<hipGraph_t, hipGraph_t, hipGraphDestroy>;
template <typename F>
int capture_graph(Ctx* c, hipStream_t s, DevGraphExec& exec, const char* end_text, F&& enqueue) {
    exec = DevGraphExec();
    HIPC(c, hipStreamSynchronize(s));
    HIPC(c, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    DevGraph g;
    hipError_t e = hipStreamEndCapture(s, &g.h);
    if (rc) return rc;
    if (e != hipSuccess || !g) return fail(c, MPST_ERR_DEVICE, end_text, hipGetErrorString(e));
    HIPC(c, hipGetLastError());     // a launch rejected during capture (bad configuration) surfaces here
    if ((e = hipGraphInstantiate(&exec.h, g, nullptr, nullptr, 0)) != hipSuccess) {
        exec.h = nullptr;
        return fail(c, MPST_ERR_DEVICE, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
    }
    return 0;
}

// What a sweep left in context c, read where its stream has just been synchronised.  read_scalars: the device scalars (a marked
// sweep reads them, redoes its rest and reads them again); read_back: with those, the subspace solver's counters and the bond
// dimensions (st->seconds is the caller's).  Device errors are reported on `rep` (a batch: its lead).
int read_scalars(Ctx* c, Ctx* rep, DevScalars* sc) {
    HIPC(rep, hipMemcpy(sc, c->ws.sc, sizeof *sc, hipMemcpyDeviceToHost));
    return 0;
}
int read_back(Ctx* c, Ctx* rep, const DevScalars* sc, mpst_sweep_stats* st) {
    refresh_ss_counts(c);
    std::vector<int32_t> chi(c->T + 1);
    HIPC(rep, hipMemcpy(chi.data(), c->mps.chi, chi.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    st->svd_status = sc->status;
    st->max_chi = *std::max_element(chi.begin(), chi.end());
    st->eig_sweeps_total = sc->eig_sweeps_total;
    st->eig_fallbacks = sc->eig_fallbacks;
    c->rebuild_steps = sc->rebuild_steps;
    if (sc->status) c->caches_valid = false;        // the state after a failed bond is unspecified: set_mps + build_caches to go on
    return 0;
}

int check_ready(Ctx* c) {
    if (!c) return MPST_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    return ensure_workspace(c);
}

int host_chi(Ctx* c, std::vector<int32_t>& chi, int32_t* ls) {
    chi.resize(c->T + 1);
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(chi.data(), c->mps.chi, (size_t)(c->T + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(ls, c->mps.label_site, sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

// evaluation chain into scratch: yhat on the device in c->ev.yeval ([N][C]).  One walk from each end of the chain to the label site,
// ping-pong between two scratch rows; in the element-typed context the step is k_tenv and the rows' exponents travel along.
int enqueue_eval(Ctx* c, int which) {
    const View v = make_view(c, which);
    if (v.N <= 0) return fail(c, MPST_ERR_INVALID, "data set %d is empty", which);
    std::vector<int32_t> chi; int32_t p;
    if (int rc = host_chi(c, chi, &p)) return rc;
    const TView t = c->typed ? make_tview(c, which) : TView{};
    EvalWs& e = c->ev;
    const int T = c->T;
    const double *Lc = nullptr, *Rc = nullptr;
    const int32_t *Lx = nullptr, *Rx = nullptr;
    auto step = [&](int j, int left, DevBuf<double>* row, DevBuf<int32_t>* xrow, int q, bool first, const double** last, const int32_t** xlast) {
        const double* prev = first ? nullptr : row[q ^ 1].h;
        const int mode = left ? ENV_M_SITE : ENV_M_SITE_T, prev_bond = left ? j : j + 1, out_bond = left ? j + 1 : j;
        if (c->typed) launch_tenv(t, j, left, prev, first ? nullptr : xrow[q ^ 1].h, prev_bond, mode, out_bond, row[q], xrow[q], c->stream);
        else launch_env(v, j, left, prev, prev_bond, mode, out_bond, row[q], c->stream);
        *last = row[q];
        *xlast = xrow[q];
    };
    for (int j = 0, q = 0; j < p; ++j, q ^= 1) step(j, 1, e.chainL, e.xchainL, q, j == 0, &Lc, &Lx);
    for (int j = T - 1, q = 0; j > p; --j, q ^= 1) step(j, 0, e.chainR, e.xchainR, q, j == T - 1, &Rc, &Rx);
    if (c->typed) launch_teval_final(t, Lc, Lx, Rc, Rx, e.yeval, c->stream);
    else launch_eval_final(v, Lc, Rc, e.yeval, c->stream);
    return 0;
}

// mpst_eval and mpst_classify: the chain, then the reduction (sums, confusion counts, predictions), waited for
int run_eval(Ctx* c, int which) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (which != 0 && which != 1) return fail(c, MPST_ERR_INVALID, "which must be 0 or 1");
    if ((rc = enqueue_eval(c, which))) return rc;
    EvalWs& e = c->ev;
    if (c->typed) launch_teval_reduce(make_tview(c, which), e.yeval, e.out3, e.conf, e.pred, c->stream);
    else launch_eval_reduce(make_view(c, which), e.yeval, e.out3, e.conf, e.pred, c->stream);
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- the sweep runner ---------------------------------------------------------------------------------------------------------
// `body` between the context's two events, waited for: *ms receives its device time.  body returns 0 or an error it has reported.
template <typename Body>
int timed(Ctx* c, float* ms, Body&& body) {
    HIPC(c, hipEventRecord(c->ev_start, c->stream));
    if (int rc = body()) return rc;
    HIPC(c, hipGetLastError());         // launch-time failures of the enqueues of body
    HIPC(c, hipEventRecord(c->ev_stop, c->stream));
    HIPC(c, hipEventSynchronize(c->ev_stop));
    HIPC(c, hipEventElapsedTime(ms, c->ev_start, c->ev_stop));
    prof_collect(c);
    return 0;
}

// the four copies of the snapshot, one list for both directions
int Snapshot::copies(Ctx* c, bool restore) {
    const size_t nchi = (size_t)c->T + 1;
    const struct { void *live, *kept; size_t bytes; } list[4] = {
        {c->mps.sites.h, sites.h, (size_t)c->mps.site_stride * c->T * c->esz},
        {c->mps.chi.h, chi.h, nchi * sizeof(int32_t)},
        {c->mps.label_site.h, chi.h + nchi, sizeof(int32_t)},
        {c->ws.sc.h, sc.h, sizeof(DevScalars)}};
    for (const auto& e : list)
        HIPC(c, hipMemcpyAsync(restore ? e.live : e.kept, restore ? e.kept : e.live, e.bytes, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}
int ensure_snapshot(Ctx* c) {
    if (c->ws.snap) return 0;
    Snapshot n;
    int rc;
    if ((rc = dalloc_e(c, n.sites, c->mps.site_stride * c->T)) || (rc = dalloc(c, n.chi, c->T + 2)) || (rc = dalloc(c, n.sc, 1))) return rc;
    c->ws.snap = std::move(n);
    return 0;
}

// the bonds of a sweep from its k0-th on (k0 > 0: the state is that after bond k0 - 1, the recovery of a marked sweep)
int enqueue_sweep(Ctx* c, const View& v, int k0 = 0) {
    if (int rc = enqueue_reset_status(c)) return rc;
    c->ynext_lid = -1;
    // unless the tensor is rescaled first or the caches are rebuilt in between, bond k+1's tensor is assembled by bond k's last launch
    const int nb = c->T - 1;
    // the rebuilds ride beside the eigensolver, a row per bond, and close with a walk of two steps (a sweep from its first bond only: the
    // recovery of a marked sweep runs the six-launch chain and keeps the full walks)
    const bool side = k0 == 0 && rebuild_side_on(c, v);
    const int first = side ? rebuild_side_first(c->T) : 0;
    bool have = false;
    for (int k = k0; k < 2 * nb; ++k) {
        const bool rebuild_after = c->opt.rebuild_caches && k == nb - 1;
        const BondSlot b = (v.rescale_before || rebuild_after) ? bond_slot(k, nb).unchained() : bond_slot(k, nb);
        if (int rc = enqueue_bond(c, v, b, have, k, side)) return rc;
        have = assembles_next(b, c->ws.fused);
        if (rebuild_after) enqueue_caches(c, v, 0, first);      // :770
    }
    if (c->opt.rebuild_caches) enqueue_caches(c, v, c->T - 1, first);                  // :804
    return 0;
}

// Four-launch chain: a tail launch whose verification failed (clustered kept eigenvalues: the case k_eig_fin hands to its Jacobi
// solver) has marked the sweep or the bond (DevScalars::redo > 0) and left the MPS, the caches and the chained tensor as the bond
// before it left them; so did every tail launch after it.  What is left to do - `enqueue`, given a fresh View: the rest of the sweep,
// or the same bond again - runs on the six-launch chain, plain stream; *sc receives what it left.
template <typename Enqueue>
int finish_marked(Ctx* c, DevScalars* sc, Enqueue&& enqueue) {
    c->tail_redos++;
    const int tail_fallbacks = sc->eig_fallbacks, side_steps = sc->rebuild_steps;
    Chain4Hold hold(c);
    if (int rc = enqueue(make_view(c, MPST_TRAIN))) return rc;
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    if (int rc = read_scalars(c, c, sc)) return rc;
    sc->eig_fallbacks += tail_fallbacks;
    sc->rebuild_steps += side_steps;        // (the rows rebuilt before the mark; the recovery itself rebuilds with full walks)
    return 0;
}

// the error a sweep returns for a non-zero device status
int sweep_failure(Ctx* c, const DevScalars& sc) {
    if (sc.status == MPST_ERR_DEVICE && c->use_ipc) {
        c->use_ipc = false;         // flags / epochs / slots are in an undefined cross-rank state: never reuse them
        c->ipc_dead = true;
        return fail(c, MPST_ERR_DEVICE, "the one-shot all-reduce timed out waiting for a peer (MPST_AR_TIMEOUT_S): rank %d of %d saw rank %d's flag at epoch %d while waiting "
                    "for one of the %llu calls issued so far; the path is retired until the inboxes are exported again", c->rank, c->nranks, sc.pad[0], sc.pad[1],
                    (unsigned long long)c->ar_epoch);
    }
    return fail(c, MPST_ERR_SVD, "bond-tensor decomposition failed (non-finite spectrum or eigensolver did not converge)");
}

// ---- batches: errors are reported on the lead, ctxs[0] --------------------------------------------------------------------------
int forward_error(Ctx* lead, const Ctx* member, int rc) {
    if (member != lead) lead->err = member->err;
    return rc;
}
// What mpst_sweep_batch and mpst_classify_batch ask of every member: there, once, ready (its own error forwarded), on the lead's
// device and of the caller's shape - shape(c, k) returns 0 or the error it has reported on the lead - and its stream idle.
template <typename Shape>
int batch_members(void* const* ctxs, int K, Shape&& shape) {
    Ctx* c0 = (Ctx*)ctxs[0];
    for (int k = 0; k < K; ++k) {
        Ctx* c = (Ctx*)ctxs[k];
        if (!c) return fail(c0, MPST_ERR_INVALID, "context %d is NULL", k);
        for (int j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return fail(c0, MPST_ERR_INVALID, "context %d appears twice", k);
        if (int rc = check_ready(c)) return forward_error(c0, c, rc);
        if (int rc = shape(c, k)) return rc;
        HIPC(c0, hipStreamSynchronize(c->stream));
    }
    HIPC(c0, hipSetDevice(c0->device));
    return 0;
}

// K independent fits of one shape advanced by ONE launch chain (hyper-parameter candidates, CV folds, restarts: what the
// reference farms out with @distributed, tuning.jl).  Every launch of the headline chain carries all K fits (blockIdx.z), so the
// kernel count per sweep is that of one fit; results are those of K separate mpst_sweep calls, bit for bit.
// batch_prepare: validation and (if the batch is new) capture of its graph; batch_run: replay and read-back.
int batch_prepare(void* const* ctxs, int32_t K) {
    if (!ctxs || K < 1 || K > 64) return fail(nullptr, MPST_ERR_INVALID, "mpst_sweep_batch: 1..64 contexts");
    Ctx* c0 = (Ctx*)ctxs[0];
    if (!c0) return MPST_ERR_INVALID;
    if (hipSetDevice(c0->device) != hipSuccess) return fail(c0, MPST_ERR_DEVICE, "cannot select device %d", c0->device);
    int rc = batch_members(ctxs, K, [&](Ctx* c, int k) {
        if (!c->caches_valid) return fail(c0, MPST_ERR_INVALID, "context %d: call mpst_build_caches first", k);
        if (c->host_label_site != c->T - 1) return fail(c0, MPST_ERR_INVALID, "context %d: a sweep starts with the label index on the last site", k);
        if (!batchable(c))
            return fail(c0, MPST_ERR_UNSUPPORTED, "context %d: mpst_sweep_batch runs the headline chain only (Float64, d*chi_max <= 128, <= 8192 series, one rank, "
                                                 "update_iters = 1, no track_cost / rebuild_caches / profiling)", k);
        // the fits may differ in their series (N, class counts, tiles: every kernel reads those from the fit's own View, the grids are sized
        // for the largest fit); whatever fixes an order of summation is either the context's (b2_ksplit, b2_nw, b2_norm_parts) or shared
        const bool same = c->device == c0->device && c->T == c0->T && c->d == c0->d && c->C == c0->C && c->mps.cap == c0->mps.cap &&
                          c->opt.loss == c0->opt.loss && c->opt.train_classes_separately == c0->opt.train_classes_separately &&
                          c->opt.chi_max == c0->opt.chi_max && c->ws.b2_ksplit == c0->ws.b2_ksplit && (c->batch_hint > 1) == (c0->batch_hint > 1) && c->ws.b2_norm_parts == c0->ws.b2_norm_parts;
        if (!same) return fail(c0, MPST_ERR_UNSUPPORTED, "context %d differs in shape from context 0 (T, d, C, capacity, chi_max, loss, gradient shares): batch fits of one shape", k);
        return 0;
    });
    if (rc) return rc;
    BatchLead& b = c0->lead;
    if (b.batch_cap < K) {
        b.batch_key.clear();
        b.batch_cap = 0;
        if ((rc = dalloc(c0, b.batch_views, (int64_t)2 * K))) return rc;
        b.batch_cap = K;
    }
    std::vector<std::pair<uint64_t, uint64_t>> key;
    for (int k = 0; k < K; ++k) key.push_back({((Ctx*)ctxs[k])->uid, ((Ctx*)ctxs[k])->epoch});
    if (b.batch_graph && key == b.batch_key) return 0;
    View v0 = make_view(c0, MPST_TRAIN);         // the launchers' geometry: the shared shape, and the tiles of the largest fit
    std::vector<View> hv((size_t)2 * b.batch_cap);
    for (int k = 0; k < K; ++k) {
        Ctx* c = (Ctx*)ctxs[k];
        v0.ntiles = std::max(v0.ntiles, c->ds[MPST_TRAIN].ntiles);
        hv[k] = make_view(c, MPST_TRAIN);
        View vg = hv[k];                    // the Gram launch reads the loss pieces and the gradient-norm pieces k_grad_s left
        vg.n_lossp = c->ws.b2_ksplit;
        vg.n_norm_part = c->ws.b2_norm_parts;
        hv[(size_t)b.batch_cap + k] = vg;
    }
    b.batch_key.clear();                  // the views the old graph reads are overwritten from here on
    HIPC(c0, hipMemcpy(b.batch_views, hv.data(), hv.size() * sizeof(View), hipMemcpyHostToDevice));
    const View* dv = b.batch_views;
    const View* dvg = b.batch_views + b.batch_cap;
    hipStream_t s = c0->stream;
    auto enqueue_batch = [&]() -> int {
        for (int k = 0; k < K; ++k) {
            const hipError_t em = hipMemsetAsync(&((Ctx*)ctxs[k])->ws.sc.h->status, 0, 12, s);
            if (em != hipSuccess) return fail(c0, MPST_ERR_DEVICE, "capture of the batched sweep failed: %s", hipGetErrorString(em));
        }
        const int nb = c0->T - 1;
        bool have = false;
        for (int q = 0; q < 2 * nb; ++q) {
            const BondSlot bs = bond_slot(q, nb);
            const int lid = bs.lid, left = bs.going_left, chain = bs.chains_into_next ? 1 : 0;
            if (!have) launch_bt_assemble_b(v0, dv, K, lid, s);
            have = assembles_next(bs, true);
            launch_yhat_s_b(v0, dv, K, lid, s);
            launch_grad_s_b(v0, dv, K, lid, s);
            launch_gram_upd_b(v0, dvg, K, lid, left, 1, s);
            launch_eig_b(v0, dv, K, lid, left, 0, s);
            launch_eig_b(v0, dv, K, lid, left, 2, s);
            launch_env_split_b(v0, dv, K, lid, left, chain, s);
        }
        return 0;
    };
    if ((rc = capture_graph(c0, s, b.batch_graph, "capture of the batched sweep failed: %s", enqueue_batch))) return rc;
    b.batch_key = key;
    return 0;
}
int batch_run(void* const* ctxs, int32_t K, mpst_sweep_stats* out) {
    Ctx* c0 = (Ctx*)ctxs[0];
    HIPC(c0, hipSetDevice(c0->device));
    float ms = 0.f;
    int rc = timed(c0, &ms, [&]() -> int {
        HIPC(c0, hipGraphLaunch(c0->lead.batch_graph, c0->stream));
        return 0;
    });
    if (rc) return rc;
    int failed = -1;
    for (int k = 0; k < K; ++k) {
        DevScalars sc;
        mpst_sweep_stats st{};
        if ((rc = read_scalars((Ctx*)ctxs[k], c0, &sc)) || (rc = read_back((Ctx*)ctxs[k], c0, &sc, &st))) return rc;
        st.seconds = 1e-3 * ms;                    // of the whole batch: the fits advance together
        if (out) out[k] = st;
        if (sc.status && failed < 0) failed = k;
    }
    if (failed >= 0) return fail(c0, MPST_ERR_SVD, "bond-tensor decomposition failed in fit %d of the batch (its svd_status is set; the other fits are intact)", failed);
    return 0;
}

// ---- data sets: validate, plan (mpst_dataset_plan.h), commit ----------------------------------------------------------------
// mpst_set_dataset and mpst_encode_[split_]dataset run every check that can reject the call before they touch the context: a
// rejected call leaves it exactly as it was.  The commit releases the old set, builds the new one aside and moves it in complete; an
// allocation or a copy that fails in between leaves the set empty (N = 0, no buffers), never N > 0 over missing buffers.
bool dtype_is_f32(int dtype) { return dtype == MPST_F32 || dtype == MPST_C64; }

// dst[b][a] = src[a][b] over rows of `row` bytes: series-major [N][T][row] <-> site-major [T][N][row]
void transpose_rows(void* dst, const void* src, int64_t A, int64_t B, size_t row) {
    for (int64_t a = 0; a < A; ++a)
        for (int64_t b = 0; b < B; ++b) memcpy((char*)dst + ((size_t)b * A + a) * row, (const char*)src + ((size_t)a * B + b) * row, row);
}

// the element type of a context is fixed by its first data set (or mpst_set_dtype) and can only change once both are gone
int dtype_validate(Ctx* c, int which, int dtype) {
    if (dtype != MPST_F64 && dtype != MPST_F32 && dtype != MPST_C128 && dtype != MPST_C64) return fail(c, MPST_ERR_INVALID, "unknown dtype %d", dtype);
    const bool other = c->ds[which ^ 1].N > 0 || c->have_mps;
    if (c->have_dtype && dtype != c->dtype && other)
        return fail(c, MPST_ERR_INVALID, "dtype %d disagrees with the context's element type %d (data sets and MPS share one element type, opts.dtype)", dtype, c->dtype);
    return 0;
}
void set_ctx_dtype(Ctx* c, int dtype) {
    if (!c->have_dtype || dtype != c->dtype) c->ws_ready = c->eval_ready = false;
    c->dtype = dtype;
    c->have_dtype = true;
    c->zw = (dtype == MPST_C128 || dtype == MPST_C64) ? 2 : 1;
    c->esz = (size_t)(dtype_is_f32(dtype) ? 4 : 8) * c->zw;
    c->typed = dtype != MPST_F64 || getenv("MPST_TYPED") != nullptr;
}

bool fits_sigmoid(const mpst_encode_opts* eo) { return eo->sigmoid_transform && eo->fit_sigmoid && !eo->is_test; }
int preprocess_validate(Ctx* c, const mpst_encode_opts* eo, int64_t N, int32_t T) {
    if (eo->fit_sigmoid && eo->is_test) return fail(c, MPST_ERR_INVALID, "fit_sigmoid: the RobustSigmoid is fitted on the training set only");
    if (eo->sigmoid_transform && !fits_sigmoid(eo) && !(eo->iqr > 0.0)) return fail(c, MPST_ERR_INVALID, "robust sigmoid needs iqr > 0");
    if (fits_sigmoid(eo) && N * (int64_t)T > 0x7fffffffll) return fail(c, MPST_ERR_UNSUPPORTED, "fit_sigmoid sorts at most 2^31 - 1 values");
    return 0;
}

// the verdict of mpst_encode_plan.h on a request's basis, reported like every other check
int basis_validate(Ctx* c, const EncodeBasis& basis, int32_t T, int32_t d) {
    const EncodeReject r = encode_basis_validate(basis, T, d);
    return r.code ? fail(c, r.code, "%s", r.text.c_str()) : 0;
}

// What mpst_set_dataset (encoded values of the given dtype) and, with eo set, the mpst_encode_*dataset entry points (raw values through
// eo into `basis`; dtype from the context or the basis) ask for
struct DataSetRequest {
    int which;
    const int32_t* label_idx;
    int64_t N;
    int32_t T, d, C;
    int dtype;
    const int64_t* n_global_per_class;
    bool have_values;
    mpst_encode_opts* eo = nullptr;
    EncodeBasis basis;
};

// Every check that can reject the call, in the order the entry points report them; fills r.dtype of an encode call and the plan.
// Reads the context, changes nothing of it.
int dataset_validate(Ctx* c, DataSetRequest& r, DataSetPlan* plan) {
    if (int rc = r.eo ? basis_validate(c, r.basis, r.T, r.d) : 0) return rc;
    if (r.which != MPST_TRAIN && r.which != MPST_TEST) return fail(c, MPST_ERR_INVALID, "which must be 0 (train) or 1 (test)");
    if (r.eo) {
        // the element type: what mpst_set_dtype / the other data set fixed (opts.dtype), else the basis' own (Float64 / ComplexF64)
        const bool bcx = r.basis.is_complex();
        r.dtype = c->have_dtype ? c->dtype : (bcx ? MPST_C128 : MPST_F64);
        if (bcx && (r.dtype == MPST_F64 || r.dtype == MPST_F32))
            return fail(c, MPST_ERR_INVALID, "Using a complex valued encoding but the MPS is real. If using a complex-valued custom encoding, set 'dtype <: Complex' in MPSOptions");   // RealRealHighDimension.jl:462-464
    }
    if (int rc = dtype_validate(c, r.which, r.dtype)) return rc;
    if (r.N < 0 || r.T < 2 || r.d < 1 || r.C < 1) return fail(c, MPST_ERR_INVALID, "bad data set dimensions");
    if ((c->T && c->T != r.T) || (c->d && c->d != r.d) || (c->C && c->C != r.C)) {
        if (c->have_mps || c->ds[r.which ^ 1].N > 0)
            return fail(c, MPST_ERR_INVALID, "data set dimensions (T=%d,d=%d,C=%d) disagree with the context (T=%d,d=%d,C=%d)", r.T, r.d, r.C, c->T, c->d, c->C);
    }
    plan->counts.assign(r.C, 0);
    if (r.N == 0) return 0;         // an empty set: no pointer is read
    if (!r.have_values || !r.label_idx) return fail(c, MPST_ERR_INVALID, "NULL data pointer");
    const char* e = getenv("MPST_PARTS");
    const LabelVerdict v = plan_dataset(r.label_idx, r.N, r.C, r.n_global_per_class, e ? std::max(1, atoi(e)) : 0, plan);
    if (v.what == LabelVerdict::OUT_OF_RANGE) return fail(c, MPST_ERR_INVALID, "label_idx[%lld] = %d out of range", (long long)v.index, v.label);
    if (v.what == LabelVerdict::UNSORTED) return fail(c, MPST_ERR_INVALID, "Training data must be sorted by class!");  // :624
    return r.eo ? preprocess_validate(c, r.eo, r.N, r.T) : 0;
}

template <typename T>
int upload(Ctx* c, DevBuf<T>& dst, const std::vector<T>& src) {
    if (int rc = dalloc(c, dst, (int64_t)src.size())) return rc;
    if (!src.empty()) HIPC(c, hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// The commit of a validated request: the context takes its element type and dimensions and forgets the old set `which` (released
// before anything is allocated: the peak is one set, not two); *n receives the plan's tables, the labels and room for the states.
int dataset_commit(Ctx* c, const DataSetRequest& r, const DataSetPlan& p, DataSet* n) {
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    set_ctx_dtype(c, r.dtype);
    c->T = r.T; c->d = r.d; c->C = r.C;
    c->ds[r.which] = DataSet();
    if (r.which == MPST_TRAIN) c->ws_ready = c->caches_valid = false;       // caches, yhat, partials are sized by the training set
    c->eval_ready = false;
    c->epoch++;
    n->N = r.N;
    n->counts = p.counts;
    if (r.N == 0) return 0;
    n->Nglobal = p.Nglobal;
    n->ntiles = (int32_t)p.tiles.size();
    n->nchunks = (int32_t)p.chunks.size();
    int rc;
    if ((rc = dalloc_e(c, n->phi, r.N * r.T * r.d)) || (rc = dalloc(c, n->label, r.N))) return rc;
    HIPC(c, hipMemcpy(n->label, r.label_idx, (size_t)r.N * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = upload(c, n->tiles, p.tiles)) || (rc = upload(c, n->chunks, p.chunks)) || (rc = upload(c, n->cls_chunk_off, p.cls_chunk_off)) ||
        (rc = upload(c, n->cls_off, p.cls_off)) || (rc = upload(c, n->inv_count, p.inv_count)))
        return rc;
    for (int pk = 0; pk < 2; ++pk) {
        n->nparts[pk] = (int32_t)p.parts[pk].size();
        if ((rc = upload(c, n->parts[pk], p.parts[pk])) || (rc = upload(c, n->part_off[pk], p.part_off[pk]))) return rc;
    }
    return 0;
}

// The one front end of the three entry points.  fill(phi) writes the states ([T][N][d] elements of the context's type) of a non-empty
// set; the set enters the context once it is complete.
template <typename Fill>
int dataset_set(Ctx* c, DataSetRequest& r, Fill fill) {
    DataSetPlan plan;
    if (int rc = dataset_validate(c, r, &plan)) return rc;
    DataSet n;
    if (int rc = dataset_commit(c, r, plan, &n)) return rc;
    if (int rc = r.N > 0 ? fill((double*)n.phi) : 0) return rc;
    c->ds[r.which] = std::move(n);
    return 0;
}

// `launch` (returns a hipError_t) timed: its device time is added to *seconds
template <typename Launch>
int timed_launch(Ctx* c, double* seconds, Launch launch) {
    float ms = 0.f;
    if (int rc = timed(c, &ms, [&]() -> int { HIPC(c, launch()); return 0; })) return rc;
    *seconds += 1e-3 * ms;
    return 0;
}

// preprocessing + encoding of X[N][T] into dphi ([T][N][d] doubles, or (re, im) pairs for the Fourier basis): shared by
// mpst_encode_dataset (dphi = the data set's product states) and mpst_encode_values (dphi = scratch, copied out)
// `basis` has passed basis_validate, eo preprocess_validate.  The basis' tables (mpst_encode_plan.h) are uploaded for the call - nothing
// reads them once the states are written -, so the context holds nothing of a call that fails later.
int encode_core(Ctx* c, const double* X, int64_t N, int32_t T, int32_t d, mpst_encode_opts* eo, const EncodeBasis& basis, double* dphi,
                double* oob_fix, double* seconds) {
    int rc;
    const EncodeTables tab = encode_tables(basis, T, d);
    DevBuf<double> tf64, dX, part, lohi, fix;       // released on every exit path, the HIPC early returns included
    DevBuf<int32_t> ti32;
    if ((!tab.f64.empty() && (rc = upload(c, tf64, tab.f64))) || (!tab.i32.empty() && (rc = upload(c, ti32, tab.i32)))) return rc;
    if ((rc = dalloc(c, dX, N * T)) || (rc = dalloc(c, part, 512)) || (rc = dalloc(c, lohi, 2))) return rc;
    const bool test = eo->is_test != 0;
    if (test && eo->rescale_out_of_bounds && (rc = dalloc(c, fix, 2 * N))) return rc;
    HIPC(c, hipMemcpy(dX, X, (size_t)N * T * sizeof(double), hipMemcpyHostToDevice));
    double secs = 0.0;
    if (fits_sigmoid(eo)) {
        // Normalization.fit(RobustSigmoid, X_train) (utils.jl:174): median and quartiles of all values from a device sort
        DevBuf<double> sorted, q3;
        DevBuf<uint8_t> tmp;
        const size_t tb = order_stats_temp_bytes(N * T);
        if ((rc = dalloc(c, sorted, N * T)) || (rc = dalloc(c, q3, 3)) || (rc = dalloc(c, tmp, (int64_t)tb))) return rc;
        if ((rc = timed_launch(c, &secs, [&] { return launch_order_stats(dX, sorted, tmp, tb, N * T, q3, c->stream); }))) return rc;
        double h3[3];
        HIPC(c, hipMemcpy(h3, q3, sizeof h3, hipMemcpyDeviceToHost));
        eo->median = h3[0];
        eo->iqr = h3[2] - h3[1];
        if (!(eo->iqr > 0.0)) return fail(c, MPST_ERR_INVALID, "robust sigmoid needs iqr > 0 (the training data has iqr = %g)", eo->iqr);
    }
    if (test || !eo->minmax) {
        const double h[2] = {eo->lo, eo->hi};
        HIPC(c, hipMemcpy(lohi, h, sizeof h, hipMemcpyHostToDevice));
    }
    EncDev e{};
    e.N = N; e.T = T; e.d = d;
    e.kind = basis.kind;
    e.basis = basis.family();
    e.fourier = basis.is_complex();
    e.sigmoid = eo->sigmoid_transform; e.minmax = eo->minmax;
    e.med = eo->median; e.s = eo->iqr / 1.35;
    e.lb = eo->data_lb; e.ub = eo->data_ub; e.a = eo->range_a; e.b = eo->range_b;
    const int bd = basis.aux_dim(d);
    e.nrm = std::sqrt(std::sqrt((2 * bd + 1) / 2.0) * bd);
    e.lohi = lohi; e.fix = fix;
    auto f64 = [&](const EncodeSpan& s) { return s.off < 0 ? nullptr : (const double*)tf64 + s.off; };
    auto i32 = [&](const EncodeSpan& s) { return s.off < 0 ? nullptr : (const int32_t*)ti32 + s.off; };
    e.bins = f64(tab.bins); e.bin_stride = tab.bin_stride;
    if (const mpst_split_opts* sp = basis.sp()) { e.nbins = sp->nbins; e.aux_dim = sp->aux_dim; }
    e.kde_lo = f64(tab.kde_lo); e.kde_step = f64(tab.kde_step); e.kde_minx = f64(tab.kde_minx); e.kde_scale = f64(tab.kde_scale);
    e.kde_coef = f64(tab.kde_coef); e.kde_cvecs = f64(tab.kde_cvecs); e.kde_zero = i32(tab.kde_zero);
    if (const mpst_kde_opts* kd = basis.kd()) { e.kde_npoints = kd->npoints; e.kde_per_site = kd->per_site; }
    e.proj_tab = i32(tab.proj_tab); e.proj_inv = f64(tab.proj_inv);
    if ((rc = timed_launch(c, &secs, [&] {
            launch_encode(e, dX, dphi, part, lohi, fix, !test && eo->minmax, c->stream);
            return hipGetLastError();
        })))
        return rc;
    if (seconds) *seconds = secs;
    if (!test && eo->minmax) {
        double h[2];
        HIPC(c, hipMemcpy(h, lohi, sizeof h, hipMemcpyDeviceToHost));
        eo->lo = h[0];
        eo->hi = h[1];
    }
    if (fix && oob_fix) HIPC(c, hipMemcpy(oob_fix, fix, (size_t)2 * N * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// the four mpst_encode_*dataset entry points: `basis` says which
int encode_dataset(void* ctx, int which, const double* X, const int32_t* label_idx, int64_t N, int32_t T, int32_t d, int32_t C,
                   mpst_encode_opts* eo, const EncodeBasis& basis, const int64_t* n_global_per_class, double* oob_fix, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (!eo) return fail(c, MPST_ERR_INVALID, "NULL encode options");
    DataSetRequest r{which, label_idx, N, T, d, C, 0, n_global_per_class, X != nullptr, eo, basis};
    return dataset_set(c, r, [&](double* dphi) {
        const bool bcx = basis.is_complex();
        if (r.dtype == (bcx ? MPST_C128 : MPST_F64)) return encode_core(c, X, N, T, d, eo, basis, dphi, oob_fix, seconds);
        // the basis' own type (fp64, real or pairs) aside, then cast to the context's
        DevBuf<double> tmp;
        int rc;
        if ((rc = dalloc(c, tmp, N * T * d * (bcx ? 2 : 1))) || (rc = encode_core(c, X, N, T, d, eo, basis, tmp, oob_fix, seconds))) return rc;
        launch_tcast(tmp, bcx ? 1 : 0, dphi, c->zw == 2, dtype_is_f32(r.dtype), N * T * d, c->stream);
        HIPC(c, hipGetLastError());
        HIPC(c, hipStreamSynchronize(c->stream));
        return 0;
    });
}

// the four mpst_encode_*values entry points: `basis` says which
int encode_values(void* ctx, const double* X, int64_t N, int32_t T, int32_t d, mpst_encode_opts* eo, const EncodeBasis& basis, void* phi_out,
                  double* oob_fix, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (!eo || !X || !phi_out) return fail(c, MPST_ERR_INVALID, "NULL argument");
    if (N <= 0 || T < 1 || d < 1 || d > 64) return fail(c, MPST_ERR_INVALID, "bad dimensions");
    int rc;
    if ((rc = basis_validate(c, basis, T, d)) || (rc = preprocess_validate(c, eo, N, T))) return rc;
    HIPC(c, hipSetDevice(c->device));
    const size_t w = (size_t)d * (basis.is_complex() ? 2 : 1);
    DevBuf<double> dphi;
    if ((rc = dalloc(c, dphi, (int64_t)(N * T * w))) || (rc = encode_core(c, X, N, T, d, eo, basis, dphi, oob_fix, seconds))) return rc;
    std::vector<double> tmp((size_t)N * T * w);
    HIPC(c, hipMemcpy(tmp.data(), dphi, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    transpose_rows(phi_out, tmp.data(), T, N, w * sizeof(double));
    return 0;
}

}  // namespace

// ===========================================================================================
extern "C" {

int mpst_version(void) { return MPST_ABI_VERSION; }

const char* mpst_last_error(void* ctx) { return ctx ? ((Ctx*)ctx)->err.c_str() : g_err.c_str(); }

int mpst_create(void** ctx, int device_id) {
    if (!ctx) return fail(nullptr, MPST_ERR_INVALID, "ctx is NULL");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, MPST_ERR_DEVICE, "no HIP device available (%s)", hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, MPST_ERR_INVALID, "device %d out of range (%d devices)", device_id, ndev);
    Ctx* c = new Ctx();
    static std::atomic<uint64_t> next_uid{1};
    c->uid = next_uid.fetch_add(1);
    c->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreate(&c->stream.h) != hipSuccess) {
        delete c;
        return fail(nullptr, MPST_ERR_DEVICE, "cannot initialise device %d", device_id);
    }
    (void)hipEventCreate(&c->ev_start.h);
    (void)hipEventCreate(&c->ev_stop.h);
    *ctx = c;
    return 0;
}

void mpst_destroy(void* ctx) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->comm && rccl_ready(nullptr)) rccl_ready(nullptr)->CommDestroy(c->comm);
    delete c;
}

int mpst_comm_unique_id(uint8_t out_id[128]) {
    ncclUniqueId id;
    static_assert(sizeof(id) == 128, "ncclUniqueId size");
    std::string why;
    Rccl* nc = rccl_ready(&why);
    if (!nc) return fail(nullptr, MPST_ERR_DEVICE, "%s", why.c_str());
    ncclResult_t r = nc->GetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, MPST_ERR_DEVICE, "ncclGetUniqueId: %s", nc->GetErrorString(r));
    memcpy(out_id, &id, 128);
    return 0;
}

int mpst_comm_init(void* ctx, const uint8_t unique_id[128], int nranks, int rank) {
    Ctx* c = (Ctx*)ctx;
    if (!c || nranks < 1 || rank < 0 || rank >= nranks) return fail(c, MPST_ERR_INVALID, "bad communicator arguments");
    HIPC(c, hipSetDevice(c->device));
    std::string why;
    Rccl* nc = rccl_ready(&why);
    if (!nc) return fail(c, MPST_ERR_DEVICE, "%s", why.c_str());
    // Only six entry points are used (ncclGetUniqueId / CommInitRank / CommDestroy / AllReduce / GetErrorString / GetVersion)
    // with ncclDouble, ncclSum and the 128-byte ncclUniqueId - unchanged across the 2.x series - so a host's copy of another
    // MINOR version (torch 2.10 ships 2.26.6 next to ROCm 7.2's 2.27.7) is accepted; another major version is not.
    if (nc->version / 10000 != NCCL_VERSION_CODE / 10000 || nc->version < 21800)
        return fail(c, MPST_ERR_DEVICE, "librccl %s has version %d, this library was built against %d (set MPST_RCCL_LIB to a matching one)",
                    nc->path.c_str(), nc->version, (int)NCCL_VERSION_CODE);
    if (c->comm) { nc->CommDestroy(c->comm); c->comm = nullptr; }
    c->nranks = nranks; c->rank = rank;
    c->force_coll = getenv("MPST_FORCE_COLLECTIVE") != nullptr;
    c->epoch++;
    ncclUniqueId id;
    memcpy(&id, unique_id, 128);
    ncclResult_t r = nc->CommInitRank(&c->comm, nranks, id, rank);
    if (r != ncclSuccess) { c->comm = nullptr; return fail(c, MPST_ERR_DEVICE, "ncclCommInitRank: %s", nc->GetErrorString(r)); }
    return 0;
}

int mpst_comm_library(char* path_out, int32_t path_cap, int32_t* version_out, int32_t* built_against_out) {
    Rccl* nc = rccl_get();
    if (version_out) *version_out = nc->version;
    if (built_against_out) *built_against_out = (int32_t)NCCL_VERSION_CODE;
    if (path_out && path_cap > 0) {
        const std::string t = nc->h ? nc->path + " (" + nc->how + ")" : nc->err;
        snprintf(path_out, (size_t)path_cap, "%s", t.c_str());
    }
    return nc->h ? 0 : MPST_ERR_DEVICE;
}

int mpst_comm_ipc_export(void* ctx, int nranks, int rank, uint8_t handle_out[64]) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !handle_out || nranks < 2 || nranks > AR_MAX_RANKS || rank < 0 || rank >= nranks)
        return fail(c, MPST_ERR_INVALID, "one-shot all-reduce: 2..%d ranks", AR_MAX_RANKS);
    int rc = check_ready(c);             // the slot size follows the gradient buffer: options, data set and MPS first
    if (rc) return rc;
    if (c->comm && (c->nranks != nranks || c->rank != rank)) return fail(c, MPST_ERR_INVALID, "rank / size disagree with the RCCL communicator");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t size");
    ipc_release(c);
    c->nranks = nranks; c->rank = rank;
    const int64_t dm = (int64_t)c->d * c->mps.cap;
    c->ipc_slot = std::max<int64_t>(2 + c->zw * c->C * dm * dm, 4 + (int64_t)c->C * c->C);
    c->ipc_slot = (c->ipc_slot + 15) & ~15ll;
    c->ipc_flag_off = (size_t)2 * nranks * c->ipc_slot * sizeof(double);
    c->ipc_ctr_off = c->ipc_flag_off + 16 * sizeof(unsigned long long);
    c->ipc_bytes = c->ipc_ctr_off + 64;
    // fine-grained device memory: peers write it and this device polls it while kernels run
    hipError_t e = hipExtMallocWithFlags((void**)&c->ipc_local.h, c->ipc_bytes, hipDeviceMallocFinegrained);
    if (e != hipSuccess) return fail(c, MPST_ERR_NOMEM, "hipExtMallocWithFlags(fine-grained, %zu bytes): %s", c->ipc_bytes, hipGetErrorString(e));
    HIPC(c, hipMemset(c->ipc_local, 0, c->ipc_bytes));
    HIPC(c, hipDeviceSynchronize());
    hipIpcMemHandle_t h;
    e = hipIpcGetMemHandle(&h, c->ipc_local);
    if (e != hipSuccess) return fail(c, MPST_ERR_DEVICE, "hipIpcGetMemHandle: %s", hipGetErrorString(e));
    memcpy(handle_out, &h, 64);
    c->ar_epoch = 0;
    c->epoch++;
    return 0;
}

int mpst_comm_ipc_attach(void* ctx, const uint8_t* all_handles) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !all_handles || !c->ipc_local) return fail(c, MPST_ERR_INVALID, "call mpst_comm_ipc_export first");
    HIPC(c, hipSetDevice(c->device));
    for (int r = 0; r < c->nranks; ++r) {
        if (r == c->rank) { c->ipc_peer[r] = c->ipc_local.h; continue; }
        hipIpcMemHandle_t h;
        memcpy(&h, all_handles + (size_t)64 * r, 64);
        hipError_t e = hipIpcOpenMemHandle(&c->ipc_peer[r], h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            c->ipc_peer[r] = nullptr;
            return fail(c, MPST_ERR_DEVICE, "hipIpcOpenMemHandle(rank %d): %s", r, hipGetErrorString(e));
        }
    }
    c->use_ipc = true;
    c->ipc_dead = false;
    c->epoch++;
    return 0;
}

int mpst_comm_select(void* ctx, int oneshot) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (oneshot && !c->ipc_peer[c->nranks > 1 ? (c->rank ^ 1) % c->nranks : 0]) return fail(c, MPST_ERR_INVALID, "inboxes are not attached");
    if (!oneshot && !c->comm) return fail(c, MPST_ERR_INVALID, "no RCCL communicator");
    c->use_ipc = oneshot != 0;
    c->epoch++;
    return 0;
}

int mpst_set_options(void* ctx, const mpst_options* o) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !o) return fail(c, MPST_ERR_INVALID, "NULL argument");
    if (o->chi_max < 1) return fail(c, MPST_ERR_INVALID, "chi_max must be >= 1");
    if (o->update_iters < 1) return fail(c, MPST_ERR_INVALID, "update_iters must be >= 1");
    if (o->loss != MPST_LOSS_KLD && o->loss != MPST_LOSS_MSE)
        return fail(c, MPST_ERR_UNSUPPORTED, "loss_grad must be KLD or MSE (Mixed exists only in the legacy ITensor path)");
    if (o->optimiser != MPST_OPT_TSGO && o->optimiser != MPST_OPT_GD)
        return fail(c, MPST_ERR_UNSUPPORTED, "Optim/OptimKit based solvers currently unimplemented for this version, set 'use_legacy_ITensor=true' in MPSOptions to enable");
    if (o->loss == MPST_LOSS_MSE && o->train_classes_separately)
        return fail(c, MPST_ERR_UNSUPPORTED, "no Loss_Grad_MSE method for TrainSeparate{true} (loss_functions.jl:561)");
    if (c->have_mps && o->chi_max > c->mps.cap)
        return fail(c, MPST_ERR_INVALID, "chi_max %d exceeds the capacity %d fixed when the MPS was set; call mpst_set_options before mpst_set_mps", o->chi_max, c->mps.cap);
    const bool resize = !c->have_opt || o->rescale_before != c->opt.rescale_before || o->update_iters != c->opt.update_iters;
    c->opt = *o;
    c->have_opt = true;
    c->epoch++;
    if (resize) c->ws_ready = false;
    return 0;
}

int mpst_set_dtype(void* ctx, int32_t dtype) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (c->ds[0].N > 0 || c->ds[1].N > 0 || c->have_mps) {
        if (c->have_dtype && dtype == c->dtype) return 0;
        return fail(c, MPST_ERR_INVALID, "mpst_set_dtype must precede the data sets and the MPS");
    }
    const int rc = dtype_validate(c, 0, dtype);
    if (!rc) set_ctx_dtype(c, dtype);
    return rc;
}

int mpst_set_dataset(void* ctx, int which, const void* phi, const int32_t* label_idx, int64_t N, int32_t T, int32_t d,
                     int32_t C, int32_t dtype, const int64_t* n_global_per_class) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    DataSetRequest r{which, label_idx, N, T, d, C, dtype, n_global_per_class, phi != nullptr};
    return dataset_set(c, r, [&](double* dphi) {
        const size_t row = (size_t)d * c->esz;
        std::vector<char> tmp((size_t)N * T * row);
        transpose_rows(tmp.data(), phi, N, T, row);
        HIPC(c, hipMemcpy(dphi, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
        return 0;
    });
}

int mpst_encode_dataset(void* ctx, int which, const double* X, const int32_t* label_idx, int64_t N, int32_t T, int32_t d,
                        int32_t C, mpst_encode_opts* eo, const int64_t* n_global_per_class, double* oob_fix, double* seconds) {
    return encode_dataset(ctx, which, X, label_idx, N, T, d, C, eo, EncodeBasis::closed(eo), n_global_per_class, oob_fix, seconds);
}

int mpst_encode_split_dataset(void* ctx, int which, const double* X, const int32_t* label_idx, int64_t N, int32_t T, int32_t d,
                              int32_t C, mpst_encode_opts* eo, const mpst_split_opts* sp, const int64_t* n_global_per_class, double* oob_fix,
                              double* seconds) {
    return encode_dataset(ctx, which, X, label_idx, N, T, d, C, eo, EncodeBasis::split(sp), n_global_per_class, oob_fix, seconds);
}

int mpst_encode_values(void* ctx, const double* X, int64_t N, int32_t T, int32_t d, mpst_encode_opts* eo, void* phi_out, double* oob_fix,
                       double* seconds) {
    return encode_values(ctx, X, N, T, d, eo, EncodeBasis::closed(eo), phi_out, oob_fix, seconds);
}

int mpst_encode_split_values(void* ctx, const double* X, int64_t N, int32_t T, int32_t d, mpst_encode_opts* eo, const mpst_split_opts* sp,
                             void* phi_out, double* oob_fix, double* seconds) {
    return encode_values(ctx, X, N, T, d, eo, EncodeBasis::split(sp), phi_out, oob_fix, seconds);
}

int mpst_encode_kde_dataset(void* ctx, int which, const double* X, const int32_t* label_idx, int64_t N, int32_t T, int32_t d,
                            int32_t C, mpst_encode_opts* eo, const mpst_kde_opts* kd, const int64_t* n_global_per_class, double* oob_fix,
                            double* seconds) {
    return encode_dataset(ctx, which, X, label_idx, N, T, d, C, eo, EncodeBasis::kde(kd), n_global_per_class, oob_fix, seconds);
}

int mpst_encode_kde_values(void* ctx, const double* X, int64_t N, int32_t T, int32_t d, mpst_encode_opts* eo, const mpst_kde_opts* kd,
                           void* phi_out, double* oob_fix, double* seconds) {
    return encode_values(ctx, X, N, T, d, eo, EncodeBasis::kde(kd), phi_out, oob_fix, seconds);
}

int mpst_encode_proj_dataset(void* ctx, int which, const double* X, const int32_t* label_idx, int64_t N, int32_t T, int32_t d,
                             int32_t C, mpst_encode_opts* eo, const mpst_proj_opts* pj, const int64_t* n_global_per_class, double* oob_fix,
                             double* seconds) {
    return encode_dataset(ctx, which, X, label_idx, N, T, d, C, eo, EncodeBasis::proj(pj), n_global_per_class, oob_fix, seconds);
}

int mpst_encode_proj_values(void* ctx, const double* X, int64_t N, int32_t T, int32_t d, mpst_encode_opts* eo, const mpst_proj_opts* pj,
                            void* phi_out, double* oob_fix, double* seconds) {
    return encode_values(ctx, X, N, T, d, eo, EncodeBasis::proj(pj), phi_out, oob_fix, seconds);
}

int mpst_get_encoded(void* ctx, int which, double* phi_out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !phi_out) return MPST_ERR_INVALID;
    if (which != MPST_TRAIN && which != MPST_TEST) return fail(c, MPST_ERR_INVALID, "which must be 0 (train) or 1 (test)");
    const DataSet& s = c->ds[which];
    if (s.N == 0) return 0;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    const size_t row = (size_t)c->d * c->esz;             // phi_out holds elements of the context's type
    std::vector<char> tmp((size_t)s.N * c->T * row);
    HIPC(c, hipMemcpy(tmp.data(), s.phi, tmp.size(), hipMemcpyDeviceToHost));
    transpose_rows(phi_out, tmp.data(), c->T, s.N, row);
    return 0;
}

// the chain of an MPS handed over from the host: the label site, the ends, every bond dimension at least 1.  *cap: the largest
static int check_chain(Ctx* c, const int32_t* chi, int32_t T, int32_t label_site, int* cap) {
    if (label_site < 0 || label_site >= T) return fail(c, MPST_ERR_INVALID, "label_site out of range");
    if (chi[0] != 1 || chi[T] != 1) return fail(c, MPST_ERR_INVALID, "chi[0] and chi[T] must be 1");
    *cap = 1;
    for (int j = 0; j <= T; ++j) {
        if (chi[j] < 1) return fail(c, MPST_ERR_INVALID, "chi[%d] < 1", j);
        *cap = std::max(*cap, (int)chi[j]);
    }
    return 0;
}

int mpst_set_mps(void* ctx, const void* const* site, const int32_t* chi, int32_t T, int32_t label_site) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !site || !chi) return fail(c, MPST_ERR_INVALID, "NULL argument");
    if (!c->have_opt) return fail(c, MPST_ERR_INVALID, "call mpst_set_options before mpst_set_mps");
    if (c->T == 0) return fail(c, MPST_ERR_INVALID, "call mpst_set_dataset before mpst_set_mps");
    if (T != c->T) return fail(c, MPST_ERR_INVALID, "MPS has %d sites, data has %d", T, c->T);
    int cap = 1;
    if (int rc = check_chain(c, chi, T, label_site, &cap)) return rc;
    cap = std::max(cap, (int)c->opt.chi_max);
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    const int d = c->d, C = c->C;
    if (cap != c->mps.cap || !c->mps.sites) {
        // the old MPS goes first, the new one is built aside and moved in complete: a failure leaves the context without one
        c->have_mps = c->ws_ready = false;
        c->mps = Mps();
        Mps m;
        m.cap = cap;
        m.site_stride = (int64_t)C * cap * d * cap;
        int rc;
        if ((rc = dalloc_e(c, m.sites, m.site_stride * T)) || (rc = dalloc(c, m.chi, T + 1)) || (rc = dalloc(c, m.label_site, 1))) return rc;
        c->mps = std::move(m);
    }
    // boundary layout (s, l, r[, c]) column-major  ->  internal [c][l][s][r]; elements of esz bytes (a pure permutation)
    const size_t esz = c->esz;
    std::vector<char> buf((size_t)c->mps.site_stride * T * esz, 0);
    for (int j = 0; j < T; ++j) {
        const int Dl = chi[j], Dr = chi[j + 1], Cj = (j == label_site) ? C : 1;
        const char* src = (const char*)site[j];
        if (!src) return fail(c, MPST_ERR_INVALID, "site[%d] is NULL", j);
        char* dst = &buf[(size_t)j * c->mps.site_stride * esz];
        for (int cc = 0; cc < Cj; ++cc)
            for (int r = 0; r < Dr; ++r)
                for (int l = 0; l < Dl; ++l)
                    for (int s = 0; s < d; ++s)
                        memcpy(dst + ((((size_t)cc * Dl + l) * d + s) * Dr + r) * esz, src + (s + (size_t)d * (l + (size_t)Dl * (r + (size_t)Dr * cc))) * esz, esz);
    }
    HIPC(c, hipMemcpy(c->mps.sites, buf.data(), buf.size(), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->mps.chi, chi, (size_t)(T + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->mps.label_site, &label_site, sizeof(int32_t), hipMemcpyHostToDevice));
    c->have_mps = true;
    c->caches_valid = false;
    c->host_label_site = label_site;
    c->epoch++;
    return 0;
}

int mpst_get_chi(void* ctx, int32_t* chi_out, int32_t* label_site) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !c->have_mps) return fail(c, MPST_ERR_INVALID, "no MPS set");
    HIPC(c, hipSetDevice(c->device));
    std::vector<int32_t> chi; int32_t ls;
    int rc = host_chi(c, chi, &ls);
    if (rc) return rc;
    if (chi_out) memcpy(chi_out, chi.data(), chi.size() * sizeof(int32_t));
    if (label_site) *label_site = ls;
    return 0;
}

int mpst_get_mps(void* ctx, void* const* site_out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !c->have_mps || !site_out) return fail(c, MPST_ERR_INVALID, "no MPS set / NULL argument");
    HIPC(c, hipSetDevice(c->device));
    std::vector<int32_t> chi; int32_t ls;
    int rc = host_chi(c, chi, &ls);
    if (rc) return rc;
    const size_t esz = c->esz;
    std::vector<char> buf((size_t)c->mps.site_stride * c->T * esz);
    HIPC(c, hipMemcpy(buf.data(), c->mps.sites, buf.size(), hipMemcpyDeviceToHost));
    const int d = c->d;
    for (int j = 0; j < c->T; ++j) {
        const int Dl = chi[j], Dr = chi[j + 1], Cj = (j == ls) ? c->C : 1;
        char* dst = (char*)site_out[j];
        if (!dst) return fail(c, MPST_ERR_INVALID, "site_out[%d] is NULL", j);
        const char* src = &buf[(size_t)j * c->mps.site_stride * esz];
        for (int cc = 0; cc < Cj; ++cc)
            for (int r = 0; r < Dr; ++r)
                for (int l = 0; l < Dl; ++l)
                    for (int s = 0; s < d; ++s)
                        memcpy(dst + (s + (size_t)d * (l + (size_t)Dl * (r + (size_t)Dr * cc))) * esz, src + ((((size_t)cc * Dl + l) * d + s) * Dr + r) * esz, esz);
    }
    return 0;
}

int mpst_build_caches(void* ctx) {
    Ctx* c = (Ctx*)ctx;
    int rc = check_ready(c);
    if (rc) return rc;
    const int32_t ls = c->host_label_site;
    // environments on both sides of the label site p: LE[0..p-1] and RE[T-1..p+1].  With the label
    // on the last site (the state fitMPS starts from) this is construct_caches(W; going_left=true).
    enqueue_caches(c, make_view(c, MPST_TRAIN), ls);
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->caches_valid = true;
    c->ynext_lid = -1;
    return 0;
}

int mpst_sweep(void* ctx, mpst_sweep_stats* out) {
    Ctx* c = (Ctx*)ctx;
    int rc = check_ready(c);
    if (rc) return rc;
    if (!c->caches_valid)
        return fail(c, MPST_ERR_INVALID, "the environment caches do not describe the current MPS / data set: call mpst_build_caches first");
    if (c->host_label_site != c->T - 1)
        return fail(c, MPST_ERR_INVALID, "a sweep starts with the label index on the last site (RealRealHighDimension.jl:19-29), it is on site %d", c->host_label_site);
    const View v = make_view(c, MPST_TRAIN);
    const bool use_graph = sweep_uses_graph(c);
    if (use_graph && (!c->sweep_graph || c->graph_epoch != c->epoch)) {
        if ((rc = capture_graph(c, c->stream, c->sweep_graph, "hipStreamEndCapture failed: %s", [&] { return enqueue_sweep(c, v); }))) return rc;
        c->graph_epoch = c->epoch;
    }
    // large bonds: no verdict is read inside the sweep (launch_eig_blocked_nosync); the state the sweep starts from is kept
    // so that a sweep in which a bond failed can be redone bond by bond
    // (one rank only: a persistent kernel that runs out of patience is a rank-local event, and a rank that redoes its sweep
    // alone would issue all-reduces its peers do not)
    const bool optimistic = c->ws.big && c->ws.blk && c->ws.big_opt && !multi(c) && c->big_cooldown == 0;
    if (c->big_cooldown > 0) c->big_cooldown--;
    if (optimistic) {
        if ((rc = ensure_snapshot(c)) || (rc = c->ws.snap.save(c))) return rc;
        c->big_opt_active = true;
    }
    struct ActiveGuard {        // whatever path leaves this function, the per-bond eigensolver path reads its verdict again
        bool& f;
        ~ActiveGuard() { f = false; }
    } active_guard{c->big_opt_active};
    float ms = 0.f;
    rc = timed(c, &ms, [&]() -> int {
        if (use_graph) HIPC(c, hipGraphLaunch(c->sweep_graph, c->stream));
        else if (int r = enqueue_sweep(c, v)) return r;
        c->ynext_lid = -1;
        if (!optimistic) return 0;
        HIPC(c, hipGetLastError());
        c->big_opt_active = false;
        const int st = blocked_eig_take_sticky(c->ws.blk, c->stream);        // the one synchronisation of the sweep
        if (st < 0) return fail(c, MPST_ERR_DEVICE, "reading the sweep's eigensolver verdict failed");
        if (!st) return 0;
        // some bond's verification failed, or a persistent tridiagonalisation gave up: everything after it ran on
        // unspecified data.  Back to the start of the sweep, caches rebuilt, bond by bond with the verdict read each time.
        c->big_redos++;
        c->big_cooldown = 4;        // whatever made the persistent kernels fail (a shared GPU, CU masking) tends to last: the next sweeps take the per-bond path
        if (int r = c->ws.snap.restore(c)) return r;
        enqueue_caches(c, v, c->T - 1);
        return enqueue_sweep(c, v);
    });
    if (rc) return rc;
    DevScalars sc;
    mpst_sweep_stats st{};
    if ((rc = read_scalars(c, c, &sc))) return rc;
    if (sc.redo > 0 && !c->chain4_hold) {
        float ms2 = 0.f;          // the rest of the sweep from the marked bond on
        const int k0 = sc.redo - 1;
        if ((rc = finish_marked(c, &sc, [&](const View& v6) { return timed(c, &ms2, [&] { return enqueue_sweep(c, v6, k0); }); }))) return rc;
        ms += ms2;
    }
    if ((rc = read_back(c, c, &sc, &st))) return rc;
    st.seconds = 1e-3 * ms;
    if (out) *out = st;
    return sc.status ? sweep_failure(c, sc) : 0;
}

int mpst_sweep_batch(void* const* ctxs, int32_t K, mpst_sweep_stats* out) {
    const int rc = batch_prepare(ctxs, K);
    return rc ? rc : batch_run(ctxs, K, out);
}

// K fits dealt over several devices (or several groups on one device): every group is one mpst_sweep_batch on its own host
// thread - no collective, nothing shared between groups.  What scales on a node: the sharded sweep replicates its eigensolver
// (70 % of a bond) on every rank, independent fits do not.
int mpst_sweep_batch_multi(void* const* ctxs, int32_t K, const int32_t* group, mpst_sweep_stats* out) {
    if (!ctxs || K < 1 || K > 512) return fail(nullptr, MPST_ERR_INVALID, "mpst_sweep_batch_multi: 1..512 contexts");
    for (int k = 0; k < K; ++k)
        if (!ctxs[k]) return fail(nullptr, MPST_ERR_INVALID, "context %d is NULL", k);
    Ctx* c0 = (Ctx*)ctxs[0];
    // groups in order of first appearance; default: one group per device
    std::vector<int32_t> keys(K);
    for (int k = 0; k < K; ++k) keys[k] = group ? group[k] : ((Ctx*)ctxs[k])->device;
    BatchGroups gr;
    const int too_large = plan_batch_groups(keys.data(), K, 64, &gr);
    const int G = (int)gr.keys.size();
    std::vector<std::vector<void*>> members(G);
    for (int g = 0; g < G; ++g) {
        for (int k : gr.index[g]) members[g].push_back(ctxs[k]);
        if (g == too_large) return fail(c0, MPST_ERR_INVALID, "group %d holds %zu contexts (at most 64 per group)", gr.keys[g], members[g].size());
        for (void* m : members[g])
            if (((Ctx*)m)->device != ((Ctx*)members[g][0])->device)
                return fail(c0, MPST_ERR_INVALID, "group %d mixes devices %d and %d: a group is one launch chain on one device", gr.keys[g],
                            ((Ctx*)members[g][0])->device, ((Ctx*)m)->device);
    }
    // a context in two groups would be swept by two host threads at once, on one stream and one set of device scalars
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return fail(c0, MPST_ERR_INVALID, "context %d appears twice", k);
    // Every group's validation and graph capture here, on the calling thread, one after the other; the threads only replay and read
    // back.  A capture in one thread is invalidated by another thread's synchronous copies (the read-back of a group that has
    // finished its sweep) - "operation failed due to a previous error during capture", one run in a dozen when two groups captured
    // side by side.
    for (int g = 0; g < G; ++g)
        if (int rc = batch_prepare(members[g].data(), (int32_t)members[g].size())) return forward_error(c0, (Ctx*)members[g][0], rc);
    std::vector<int> rc(G, 0);
    std::vector<std::vector<mpst_sweep_stats>> st(G);
    std::vector<std::thread> th;
    for (int g = 0; g < G; ++g) {
        st[g].resize(members[g].size());
        th.emplace_back([&, g] { rc[g] = batch_run(members[g].data(), (int32_t)members[g].size(), st[g].data()); });
    }
    for (auto& t : th) t.join();
    if (out)
        for (int g = 0; g < G; ++g)
            for (size_t j = 0; j < gr.index[g].size(); ++j) out[gr.index[g][j]] = st[g][j];
    for (int g = 0; g < G; ++g)
        if (rc[g]) return forward_error(c0, (Ctx*)members[g][0], rc[g]);
    return 0;
}

int mpst_set_batch_hint(void* ctx, int32_t K) {
    Ctx* c = (Ctx*)ctx;
    if (!c || K < 1) return fail(c, MPST_ERR_INVALID, "batch hint must be >= 1");
    if (K != c->batch_hint) {
        c->batch_hint = K;
        c->ws_ready = false;
        c->epoch++;
    }
    return 0;
}

int mpst_get_loss_trace(void* ctx, double* out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !out) return MPST_ERR_INVALID;
    int rc = check_ready(c);
    if (rc) return rc;
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(out, c->ws.loss_trace, (size_t)2 * (c->T - 1) * (c->opt.update_iters + 1) * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int mpst_bond_step(void* ctx, int32_t lid, int32_t going_left, mpst_bond_debug* dbg) {
    Ctx* c = (Ctx*)ctx;
    int rc = check_ready(c);
    if (rc) return rc;
    if (lid < 0 || lid > c->T - 2) return fail(c, MPST_ERR_INVALID, "lid out of range");
    if (!c->caches_valid)
        return fail(c, MPST_ERR_INVALID, "the environment caches do not describe the current MPS / data set: call mpst_build_caches first");
    if (c->host_label_site != lid && c->host_label_site != lid + 1)
        return fail(c, MPST_ERR_INVALID, "bond (%d,%d) does not hold the label index (it is on site %d)", lid, lid + 1, c->host_label_site);
    View v = make_view(c, MPST_TRAIN);
    if ((rc = enqueue_reset_status(c))) return rc;
    const BondSlot b{lid, going_left ? 1 : 0, -1, false};
    if ((rc = enqueue_bond(c, v, b))) return rc;
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    DevScalars sc;
    if ((rc = read_scalars(c, c, &sc))) return rc;
    if (sc.redo > 0) {          // the same bond again
        rc = finish_marked(c, &sc, [&](const View& v6) {
            const int r = enqueue_reset_status(c);
            return r ? r : enqueue_bond(c, v6, b);
        });
        if (rc) return rc;
    }
    refresh_ss_counts(c);
    c->host_label_site = going_left ? lid : lid + 1;
    prof_collect(c);
    if (dbg) {
        std::vector<double> lam((size_t)std::max(sc.n_spec, 1));
        HIPC(c, hipMemcpy(lam.data(), c->ws.lam, lam.size() * sizeof(double), hipMemcpyDeviceToHost));
        dbg->loss = sc.loss;
        dbg->grad_norm = sc.grad_norm;
        dbg->bt_norm = std::sqrt(sc.bt_norm2);
        dbg->chi_new = sc.n_keep;
        dbg->n_spectrum = sc.n_spec;
        dbg->eig_sweeps = sc.eig_sweeps;
        dbg->reserved = 0;
        for (int i = 0; i < sc.n_spec && i < MPST_MAX_SPECTRUM; ++i) dbg->spectrum[i] = std::sqrt(std::max(lam[i], 0.0)) * sc.inv_norm;
    }
    if (sc.status) {
        c->caches_valid = false;
        return fail(c, MPST_ERR_SVD, "bond-tensor decomposition failed at bond %d", lid);
    }
    return 0;
}

int mpst_eval(void* ctx, int which, double* mse, double* kld, double* acc, int64_t* conf) {
    Ctx* c = (Ctx*)ctx;
    int rc = run_eval(c, which);
    if (rc) return rc;
    const int64_t N = c->ds[which].N;
    double o[3];
    HIPC(c, hipMemcpy(o, c->ev.out3, sizeof o, hipMemcpyDeviceToHost));
    // multi-GPU: sums over shards
    double tot[4] = {o[0], o[1], o[2], (double)N};
    std::vector<int64_t> cf((size_t)c->C * c->C);
    HIPC(c, hipMemcpy(cf.data(), c->ev.conf, cf.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (multi(c)) {
        // sums over shards: the 4 scalars and the C x C counts (exact in fp64) travel as one message
        std::vector<double> msg(4 + cf.size());
        for (int i = 0; i < 4; ++i) msg[i] = tot[i];
        for (size_t i = 0; i < cf.size(); ++i) msg[4 + i] = (double)cf[i];
        double* dmsg = c->ev.yeval;                       // scratch of at least N*C >= ... doubles; the message is small
        if ((int64_t)msg.size() > c->ev.eval_N * c->C) return fail(c, MPST_ERR_INVALID, "evaluation scratch too small for the all-reduce message");
        HIPC(c, hipMemcpy(dmsg, msg.data(), msg.size() * sizeof(double), hipMemcpyHostToDevice));
        if ((rc = enqueue_allreduce(c, dmsg, (int64_t)msg.size(), -1))) return rc;
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, hipMemcpy(msg.data(), dmsg, msg.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < 4; ++i) tot[i] = msg[i];
        for (size_t i = 0; i < cf.size(); ++i) cf[i] = (int64_t)llround(msg[4 + i]);
    }
    if (mse) *mse = tot[0] / tot[3];
    if (kld) *kld = tot[1] / tot[3];
    if (acc) *acc = tot[2] / tot[3];
    if (conf) memcpy(conf, cf.data(), cf.size() * sizeof(int64_t));
    return 0;
}

int mpst_classify(void* ctx, int which, int32_t* pred, double* yhat) {
    Ctx* c = (Ctx*)ctx;
    int rc = run_eval(c, which);
    if (rc) return rc;
    const int64_t N = c->ds[which].N;
    if (pred) HIPC(c, hipMemcpy(pred, c->ev.pred, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (yhat) {
        if (c->typed && c->zw == 1) {           // the typed kernels keep (re, im) pairs: a real context returns the real parts
            std::vector<double> tmp((size_t)N * c->C * 2);
            HIPC(c, hipMemcpy(tmp.data(), c->ev.yeval, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < (size_t)N * c->C; ++i) yhat[i] = tmp[2 * i];
        } else {
            HIPC(c, hipMemcpy(yhat, c->ev.yeval, (size_t)N * c->C * c->zw * sizeof(double), hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

// Scoring of K models, each on its own data set `which`, in two launches for the whole batch (mpst_score.hip): what tune / evaluate
// do with every candidate x fold (hyperparameters/tuning.jl:1-207, hyperopt_utils.jl:152-231; summary.jl:4-136).  Float64 real
// contexts on one device that share T, d, C, with d * capacity <= 128; the sets' sizes and the bond dimensions may differ.  Only the
// lead context's scoring block is written: the training caches, the evaluation scratch and the streams' order are left alone.
int mpst_classify_batch(void* const* ctxs, int32_t K, int which, int32_t* const* pred, double* const* yhat, double* loss3, int64_t* conf) {
    if (!ctxs || K < 1 || K > 64) return fail(nullptr, MPST_ERR_INVALID, "mpst_classify_batch: 1..64 contexts");
    Ctx* c0 = (Ctx*)ctxs[0];
    if (!c0) return MPST_ERR_INVALID;
    if (which != 0 && which != 1) return fail(c0, MPST_ERR_INVALID, "which must be 0 or 1");
    int64_t maxN = 0, totN = 0;
    int rc = batch_members(ctxs, K, [&](Ctx* c, int k) {
        if (c->typed || c->zw == 2 || multi(c))
            return fail(c0, MPST_ERR_UNSUPPORTED, "context %d: mpst_classify_batch scores Float64 real fits on one rank (use mpst_classify)", k);
        if (!score_walk_supported(c->T, c->d, c->mps.cap, c->C))
            return fail(c0, MPST_ERR_UNSUPPORTED, "context %d: mpst_classify_batch needs d * capacity <= 128 and bond dimensions <= 64 (use mpst_classify)", k);
        if (c->device != c0->device || c->T != c0->T || c->d != c0->d || c->C != c0->C)
            return fail(c0, MPST_ERR_UNSUPPORTED, "context %d differs from context 0 in device, T, d or C: score such fits in separate calls", k);
        const int64_t n = c->ds[which].N;
        if (n <= 0) return fail(c0, MPST_ERR_INVALID, "context %d: data set %d is empty", k, which);
        maxN = std::max(maxN, n);
        totN += n;
        return 0;
    });
    if (rc) return rc;
    HIPC(c0, score_init_attrs());
    // one block: jobs | out3 [K][3] | conf [K][C][C] | yhat of every fit | pred of every fit
    const int C = c0->C;
    const size_t o_out3 = ((size_t)K * sizeof(ScoreJob) + 15) & ~(size_t)15;
    const size_t o_conf = o_out3 + (size_t)K * 3 * sizeof(double);
    const size_t o_yhat = o_conf + (size_t)K * C * C * sizeof(int64_t);
    const size_t o_pred = o_yhat + (size_t)totN * C * sizeof(double);
    const size_t bytes = o_pred + (size_t)totN * sizeof(int32_t);
    if (c0->lead.score_cap < (int64_t)bytes) {
        c0->lead.score_cap = 0;
        if ((rc = dalloc(c0, c0->lead.score_buf, (int64_t)bytes))) return rc;
        c0->lead.score_cap = (int64_t)bytes;
    }
    std::vector<ScoreJob> jobs((size_t)K);
    std::vector<int64_t> first((size_t)K + 1, 0);
    for (int k = 0; k < K; ++k) {
        Ctx* c = (Ctx*)ctxs[k];
        const DataSet& s = c->ds[which];
        ScoreJob& j = jobs[k];
        j.T = c->T; j.d = c->d; j.C = c->C; j.pad = 0;
        j.N = s.N;
        j.phi = s.phi; j.label = s.label; j.chi = c->mps.chi; j.label_site = c->mps.label_site;
        j.sites = c->mps.sites; j.site_stride = c->mps.site_stride;
        j.yhat = (double*)(c0->lead.score_buf + o_yhat) + first[k] * C;
        j.pred = (int32_t*)(c0->lead.score_buf + o_pred) + first[k];
        j.out3 = (double*)(c0->lead.score_buf + o_out3) + 3 * k;
        j.conf = (int64_t*)(c0->lead.score_buf + o_conf) + (int64_t)k * C * C;
        first[k + 1] = first[k] + s.N;
    }
    HIPC(c0, hipMemcpy(c0->lead.score_buf, jobs.data(), jobs.size() * sizeof(ScoreJob), hipMemcpyHostToDevice));
    launch_score_b((const ScoreJob*)c0->lead.score_buf.h, K, maxN, c0->stream);
    HIPC(c0, hipGetLastError());
    HIPC(c0, hipStreamSynchronize(c0->stream));
    std::vector<uint8_t> host(bytes - o_out3);
    HIPC(c0, hipMemcpy(host.data(), c0->lead.score_buf + o_out3, host.size(), hipMemcpyDeviceToHost));
    const double* h3 = (const double*)host.data();
    const int64_t* hc = (const int64_t*)(host.data() + (o_conf - o_out3));
    const double* hy = (const double*)(host.data() + (o_yhat - o_out3));
    const int32_t* hp = (const int32_t*)(host.data() + (o_pred - o_out3));
    for (int k = 0; k < K; ++k) {
        const int64_t n = first[k + 1] - first[k];
        if (loss3)
            for (int i = 0; i < 3; ++i) loss3[3 * k + i] = h3[3 * k + i] / (double)n;
        if (pred && pred[k]) memcpy(pred[k], hp + first[k], (size_t)n * sizeof(int32_t));
        if (yhat && yhat[k]) memcpy(yhat[k], hy + first[k] * C, (size_t)n * C * sizeof(double));
    }
    if (conf) memcpy(conf, hc, (size_t)K * C * C * sizeof(int64_t));
    return 0;
}

// Are the grid states the Fourier basis (src/Encodings/bases.jl:23-42: cispi(f_s x) / sqrt(d), f = 0, 1, -1, 2, -2, ...) on a uniform
// grid?  Then the kernels evaluate the conditional densities and their cumulative sums in closed form instead of streaming the
// table (k_imp_left<..., TRIG>).  Decided from the tables the caller handed over, to 1e-12; MPST_IMP_NO_TRIG=1 keeps the table path.
static bool fourier_grid(const double* gx, const double* gp, int n, int d, double* x0, double* dxu) {
    if (getenv("MPST_IMP_NO_TRIG")) return false;
    const double a = gx[0], h = (gx[n - 1] - gx[0]) / (double)(n - 1);
    if (!(h > 0.0) || !((d - 1) * h < 1.0)) return false;
    const double tolx = 1e-12 * std::max(1.0, std::max(fabs(a), fabs(gx[n - 1])));
    const double inv = 1.0 / sqrt((double)d);
    for (int k = 0; k < n; ++k) {
        if (fabs(gx[k] - (a + k * h)) > tolx) return false;
        for (int s = 0; s < d; ++s) {
            const int f = (s + 1) / 2 * ((s & 1) ? 1 : -1);
            const double ang = M_PI * (double)f * gx[k];
            if (fabs(gp[2 * ((size_t)k * d + s)] - cos(ang) * inv) > 1e-12 || fabs(gp[2 * ((size_t)k * d + s) + 1] - sin(ang) * inv) > 1e-12) return false;
        }
    }
    *x0 = a;
    *dxu = h;
    return true;
}

// Are the grid states one of the Legendre bases (bases.jl:70-108: sqrt((2s+1)/2) P_s(x), optionally over sqrt(sqrt((2d+1)/2) d)) on a
// uniform grid inside [-1, 1]?  Then p(x) is a Legendre series of degree 2d - 2 and the kernels need no table of grid states
// (k_imp_left<..., TRIG>, real models).  On success `lin` receives the linearisation table A[l][s][s'] = cn^2 kappa_s kappa_s'
// a(s, s', l), P_s P_s' = sum_l a(s, s', l) P_l, by Gauss-Legendre quadrature (64 nodes: exact far beyond degree 3 x 30).
static bool legendre_grid(const double* gx, const double* gp, int n, int d, double* x0, double* dxu, std::vector<double>* lin) {
    if (getenv("MPST_IMP_NO_TRIG") || d < 1 || d > 16) return false;
    const double a = gx[0], h = (gx[n - 1] - gx[0]) / (double)(n - 1);
    if (!(h > 0.0) || a < -1.0 - 1e-12 || gx[n - 1] > 1.0 + 1e-12) return false;
    // the closed-form prefix sums are Euler-Maclaurin truncated after the h^3 (third derivative) term; the next one,
    // h^5 / 30240 * delta p^(5), grows like (2d - 2)^10 for a Legendre series of degree 2d - 2: on a coarse grid it moves the cumulative
    // trapezoid by whole grid steps (6e-4 relative at d = 16 with 101 points).  Only grids on which it stays below 1e-12 take the
    // closed form, the rest the table path.
    if (pow(h, 5.0) * pow(2.0 * d - 2.0, 10.0) / 1e8 >= 1e-12) return false;
    const double tolx = 1e-12;
    const double nrm = sqrt(sqrt((2 * d + 1) / 2.0) * d);
    double cn = 0.0;
    std::vector<double> P(d);
    for (int k = 0; k < n; ++k) {
        const double x = gx[k];
        if (fabs(x - (a + k * h)) > tolx) return false;
        P[0] = 1.0;
        if (d > 1) P[1] = x;
        for (int m = 1; m + 1 < d; ++m) P[m + 1] = ((2 * m + 1) * x * P[m] - m * P[m - 1]) / (m + 1);
        if (k == 0) {
            // the scale of the table: with or without the norm (state 0 is the constant sqrt(1/2) cn)
            const double c0 = gp[0] / sqrt(0.5);
            if (fabs(c0 - 1.0) < 1e-12) cn = 1.0;
            else if (fabs(c0 - 1.0 / nrm) < 1e-12) cn = 1.0 / nrm;
            else return false;
        }
        for (int s = 0; s < d; ++s)
            if (fabs(gp[(size_t)k * d + s] - cn * sqrt((2.0 * s + 1.0) / 2.0) * P[s]) > 1e-12) return false;
    }
    // Gauss-Legendre nodes and weights (Newton on P_64)
    const int NG = 64, L = 2 * d - 1;
    std::vector<double> xg(NG), wg(NG);
    for (int i = 0; i < NG; ++i) {
        double x = cos(M_PI * (i + 0.75) / (NG + 0.5)), dp = 1.0;
        for (int it = 0; it < 100; ++it) {
            double p0 = 1.0, p1 = x;
            for (int m = 1; m < NG; ++m) {
                const double p2 = ((2 * m + 1) * x * p1 - m * p0) / (m + 1);
                p0 = p1;
                p1 = p2;
            }
            dp = NG * (x * p1 - p0) / (x * x - 1.0);
            const double dxn = p1 / dp;
            x -= dxn;
            if (fabs(dxn) < 1e-16) break;
        }
        xg[i] = x;
        wg[i] = 2.0 / ((1.0 - x * x) * dp * dp);
    }
    lin->assign((size_t)L * d * d, 0.0);
    std::vector<double> Q(L);
    for (int i = 0; i < NG; ++i) {
        const double x = xg[i];
        Q[0] = 1.0;
        if (L > 1) Q[1] = x;
        for (int m = 1; m + 1 < L; ++m) Q[m + 1] = ((2 * m + 1) * x * Q[m] - m * Q[m - 1]) / (m + 1);
        for (int l = 0; l < L; ++l)
            for (int s = 0; s < d; ++s)
                for (int t = 0; t < d; ++t)
                    (*lin)[((size_t)l * d + s) * d + t] += wg[i] * 0.5 * (2 * l + 1) * Q[l] * Q[s] * Q[t];
    }
    for (int l = 0; l < L; ++l)
        for (int s = 0; s < d; ++s)
            for (int t = 0; t < d; ++t)
                (*lin)[((size_t)l * d + s) * d + t] *= cn * cn * sqrt((2.0 * s + 1.0) / 2.0) * sqrt((2.0 * t + 1.0) / 2.0);
    *x0 = a;
    *dxu = h;
    return true;
}

// ---- model queries: imputation, marginal likelihoods, site conditionals ------------------------------------------------------
// Every query is: validate, get the model onto the device (the context's own, or a host model packed and uploaded for the call), plan
// the blocks (mpst_query_plan.h), run them through run_blocks.

// One imputation call as the six entry points hand it on: the arrays of the caller (host), the trajectories (mpst_impute_traj /
// mpst_impute_model_traj: K chains per instance, their uniform numbers from the caller's u or, seeded, from the device generator
// keyed by seed and row_id) and the distribution outputs (mpst_impute_dist / mpst_impute_model_dist).
struct ImputeRequest {
    const uint8_t* missing = nullptr;
    const double* grid_x = nullptr;
    const void* grid_phi = nullptr;
    int32_t ngrid = 0;
    const mpst_impute_opts* o = nullptr;
    const double* u = nullptr;
    double *x_out = nullptr, *err_out = nullptr, *seconds = nullptr;
    int32_t K = 1;
    bool seeded = false; uint64_t seed = 0;
    const int64_t* row_id = nullptr;
    bool dist = false;          // a *_dist call (also one with nq = 0 and cdf_stride = 0)
    int32_t nq = 0, cdf_stride = 0, cdf_rows = 0;
    const double* levels = nullptr;
    double *q_out = nullptr, *cdf_out = nullptr;
    bool grid_per_site() const { return o && o->grid_per_site == 1; }      // grid_phi is [T][ngrid][d]
    ImputeRequest& traj(int32_t K_, int64_t seed_, const int64_t* row_id_) {
        K = K_, seeded = u == nullptr, seed = (uint64_t)seed_, row_id = row_id_;
        return *this;
    }
    ImputeRequest& dist_outputs(int32_t nq_, const double* levels_, double* q_out_, int32_t cdf_stride_, int32_t cdf_rows_, double* cdf_out_) {
        dist = true, nq = nq_, levels = levels_, q_out = q_out_, cdf_stride = cdf_stride_, cdf_rows = cdf_rows_, cdf_out = cdf_out_;
        return *this;
    }
};
// what mpst_impute / _traj / _dist and their _model_ twins have in common
static ImputeRequest impute_request(const uint8_t* missing, const double* grid_x, const void* grid_phi, int32_t ngrid, const mpst_impute_opts* o,
                                    const double* u, double* x_out, double* err_out, double* seconds) {
    ImputeRequest r;
    r.missing = missing, r.grid_x = grid_x, r.grid_phi = grid_phi, r.ngrid = ngrid, r.o = o;
    r.u = u, r.x_out = x_out, r.err_out = err_out, r.seconds = seconds;
    return r;
}
constexpr int IMPUTE_MAX_LEVELS = 16;
// doubles of the grid table(s) a call hands over
static int64_t grid_doubles(const ImpModel& m, bool per_site, int32_t ngrid) {
    return (int64_t)(per_site ? m.T : 1) * ngrid * m.d * (m.is_complex ? 2 : 1);
}

// the two option checks imputation and site conditionals share
static int check_grid_per_site(Ctx* c, int32_t v) {
    if (v != 0 && v != 1) return fail(c, MPST_ERR_INVALID, "grid_per_site must be 0 (grid_phi[ngrid][d]) or 1 (grid_phi[T][ngrid][d]), got %d", (int)v);
    return 0;
}
static int check_levels(Ctx* c, int32_t nq, const double* levels, const double* q_out) {
    if (nq < 0 || nq > IMPUTE_MAX_LEVELS) return fail(c, MPST_ERR_INVALID, "nq must lie in 0 .. %d (got %d)", IMPUTE_MAX_LEVELS, (int)nq);
    if (nq > 0 && (!levels || !q_out)) return fail(c, MPST_ERR_INVALID, "nq > 0 needs levels[nq] and q_out[N][T][nq]");
    for (int l = 0; l < nq; ++l)
        if (!(levels[l] > 0.0 && levels[l] < 1.0)) return fail(c, MPST_ERR_INVALID, "levels[%d] = %g is not inside (0, 1)", l, levels[l]);
    return 0;
}

// the switches and the free memory the plans are cut from (mpst_query_plan.h reads neither itself)
static const char* chunk_gb_override() { return getenv("MPST_IMPUTE_CHUNK_GB"); }
static int free_device_bytes(Ctx* c, size_t* free_b) {
    size_t total_b = 0;
    HIPC(c, hipMemGetInfo(free_b, &total_b));
    return 0;
}

// One timed pass over N instances, `chunk` at a time.  enqueue(i0, count, mid) puts the launches of one block on the stream; with
// `split` it gets an event to record between its two phases, else null.  The runner owns the events, the final synchronise and
// error check, *seconds (the whole pass) and the context's impute_phase_s: the two phases summed over the blocks, (seconds, 0) without
// a split.  Hooks: what a caller does around its blocks - prepare() once inside the timed span, before() / after() each block and
// outside its phases (own_begin(): a block's first phase starts at an event of its own, not where the block before ended).
struct NoBlockHooks {
    bool own_begin() const { return false; }
    int prepare() { return 0; }
    int before(int64_t, int64_t) { return 0; }
    int after(int64_t, int64_t) { return 0; }
};
extern "C++" {
template <typename Enqueue, typename Hooks = NoBlockHooks>
static int run_blocks(Ctx* c, int64_t N, int64_t chunk, bool split, double* seconds, Enqueue&& enqueue, Hooks&& hooks = Hooks()) {
    const bool own_begin = split && hooks.own_begin();
    const size_t per = own_begin ? 3 : 2;       // events of a block: [begin,] mid, end
    std::vector<DevEvent> evs;
    auto add_event = [&]() { evs.emplace_back(); return hipEventCreate(&evs.back().h); };
    HIPC(c, hipEventRecord(c->ev_start, c->stream));
    if (int rc = hooks.prepare()) return rc;
    const int rc = for_each_block(N, chunk, [&](int64_t i0, int64_t count) -> int {
        if (int rb = hooks.before(i0, count)) return rb;
        if (own_begin) {
            HIPC(c, add_event());
            HIPC(c, hipEventRecord(evs.back(), c->stream));
        }
        if (split) {
            HIPC(c, add_event());
            HIPC(c, add_event());
        }
        if (int rl = enqueue(i0, count, split ? evs[evs.size() - 2].h : nullptr)) return rl;
        if (split) HIPC(c, hipEventRecord(evs.back(), c->stream));
        return hooks.after(i0, count);
    });
    if (rc) return rc;
    HIPC(c, hipEventRecord(c->ev_stop, c->stream));
    HIPC(c, hipGetLastError());
    HIPC(c, hipEventSynchronize(c->ev_stop));
    float ms = 0.f;
    HIPC(c, hipEventElapsedTime(&ms, c->ev_start, c->ev_stop));
    if (seconds) *seconds = 1e-3 * ms;
    c->impute_phase_s[0] = split ? 0.0 : 1e-3 * ms;
    c->impute_phase_s[1] = 0.0;
    for (size_t k = 0; k < evs.size(); k += per) {
        const hipEvent_t from = own_begin ? evs[k].h : (k == 0 ? c->ev_start : evs[k - 1].h), mid = evs[k + per - 2], end = evs[k + per - 1];
        float a = 0.f, b = 0.f;
        HIPC(c, hipEventElapsedTime(&a, from, mid));
        HIPC(c, hipEventElapsedTime(&b, mid, end));
        c->impute_phase_s[0] += 1e-3 * a;
        c->impute_phase_s[1] += 1e-3 * b;
    }
    return 0;
}
}  // extern "C++"

// what a valid request comes to, and how its instances are dealt out
struct ImputePlan {
    bool sampling, seeded;      // a sampling method; its uniform numbers come from the device generator
    int64_t ncdf, cdf_inst;     // cdf points per missing site; doubles of cdf rows per instance
    int ntrial, maxm;           // trials per site; most missing sites of an instance
    std::vector<int32_t> order; // the instances in the order they are dealt out to workgroups
    int64_t welems, chunk;      // scratch elements per instance of the large-chi environment kernel; instances per launch
};

// the checks of a request, in the order callers rely on; on the way it fills the plan's sizes (ncdf ... maxm) and raises the kernels' LDS limits
static int impute_validate(Ctx* c, const ImpModel& m, const ImputeRequest& r, ImputePlan* p) {
    const mpst_impute_opts* o = r.o;
    if (!r.missing || !r.grid_x || !r.grid_phi || !r.x_out || !o || r.ngrid < 2) return fail(c, MPST_ERR_INVALID, "NULL argument or fewer than 2 grid values");
    if (int rc = check_grid_per_site(c, o->grid_per_site)) return rc;
    if (r.dist) {
        // get_cdfs refuses every other method (imputation.jl:594-596)
        if (o->method != MPST_IMPUTE_MEDIAN) return fail(c, MPST_ERR_UNSUPPORTED, "levels and cdfs are read off the median imputer's distribution: method must be MPST_IMPUTE_MEDIAN");
        if (int rc = check_levels(c, r.nq, r.levels, r.q_out)) return rc;
        if (r.cdf_stride < 0 || r.cdf_rows < 0) return fail(c, MPST_ERR_INVALID, "cdf_stride and cdf_rows must not be negative");
        if (r.cdf_stride > 0 && !r.cdf_out) return fail(c, MPST_ERR_INVALID, "cdf_stride > 0 needs cdf_out[N][cdf_rows][ncdf]");
        if (r.cdf_stride == 0 && r.cdf_out) return fail(c, MPST_ERR_INVALID, "cdf_out must be NULL when cdf_stride is 0");
        if (r.K != 1) return fail(c, MPST_ERR_UNSUPPORTED, "levels and cdfs belong to the single-series median call");
    }
    p->ncdf = cdf_points(r.ngrid, r.cdf_stride);
    p->cdf_inst = (int64_t)r.cdf_rows * p->ncdf;
    const int method = o->method;
    if (method < MPST_IMPUTE_MEDIAN || method > MPST_IMPUTE_ITS_REJECT) return fail(c, MPST_ERR_INVALID, "unknown imputation method");
    if (o->order != MPST_IMPUTE_FORWARDS && o->order != MPST_IMPUTE_BACKWARDS) return fail(c, MPST_ERR_INVALID, "impute_order must be forwards (0) or backwards (1)");
    p->sampling = method == MPST_IMPUTE_QUANTILE || method == MPST_IMPUTE_ITS_REJECT;
    if (p->sampling && !r.u && !r.seeded) return fail(c, MPST_ERR_INVALID, "the sampling methods need the uniform numbers u[N][T][max_trials]");
    p->ntrial = method == MPST_IMPUTE_ITS_REJECT ? o->max_trials : 1;
    if (p->ntrial < 1) return fail(c, MPST_ERR_INVALID, "max_trials must be at least 1");
    p->seeded = p->sampling && !r.u && r.seeded;
    if (p->seeded && (m.T > IMPUTE_SEED_MAX_SITES || p->ntrial > IMPUTE_SEED_MAX_TRIALS))
        return fail(c, MPST_ERR_UNSUPPORTED, "the device generator's counter holds T <= %d sites and max_trials <= %d (got %d, %d): pass u",
                    IMPUTE_SEED_MAX_SITES, IMPUTE_SEED_MAX_TRIALS, m.T, p->ntrial);
    if (method == MPST_IMPUTE_ITS_REJECT && !(o->rejection_threshold >= 0.0)) return fail(c, MPST_ERR_INVALID, "rejection_threshold must be non-negative");
    if (method == MPST_IMPUTE_MEAN && o->grid_per_site)
        return fail(c, MPST_ERR_UNSUPPORTED, "the mean method re-encodes the expectation value with one closed-form basis: not with a per-site grid table "
                                             "(time-dependent encodings)");
    if (method == MPST_IMPUTE_MEAN) {
        const int mb = o->mean_basis;
        const bool real_ok = mb == MPST_BASIS_LEGENDRE || mb == MPST_BASIS_LEGENDRE_NO_NORM || mb == MPST_BASIS_UNIFORM;
        const bool cplx_ok = mb == MPST_BASIS_FOURIER || (mb == MPST_BASIS_STOUDENMIRE && m.d == 2) || (mb == MPST_BASIS_SAHAND && m.d % 2 == 0);
        if (!(m.is_complex ? cplx_ok : real_ok))
            return fail(c, MPST_ERR_UNSUPPORTED, "the mean method re-encodes on the device: Legendre / Uniform bases (real models), Fourier, "
                                                 "Stoudenmire (d = 2) or Sahand (even d) (complex models) only");
    }
    const int lim = impute_chi_limit(m.is_complex != 0, m.compute_f32 != 0);
    if (m.cap > lim || m.d > 16)
        return fail(c, MPST_ERR_UNSUPPORTED, "the imputation engine holds chi_max <= %d (this element type) and d <= 16 (got %d, %d)", lim, m.cap, m.d);
    hipError_t ea = impute_init_attrs(c->device);
    if (ea != hipSuccess) return fail(c, MPST_ERR_DEVICE, "hipFuncSetAttribute failed: %s", hipGetErrorString(ea));
    p->maxm = 0;
    for (int64_t i = 0; i < m.N; ++i) {
        int mm = 0;
        for (int j = 0; j < m.T; ++j) mm += r.missing[i * m.T + j] ? 1 : 0;
        p->maxm = std::max(p->maxm, mm);
        if (r.cdf_stride > 0 && mm > r.cdf_rows)
            return fail(c, MPST_ERR_INVALID, "instance %lld has %d missing sites, cdf_out holds cdf_rows = %d", (long long)i, mm, r.cdf_rows);
    }
    return 0;
}

// instances per launch (mpst_query_plan.h: impute_plan_block), or the verdict that not even a block of one fits
static int impute_block(Ctx* c, const ImpModel& m, const ImputeRequest& r, size_t free_b, ImputePlan* p) {
    p->welems = impute_work_elems(m.cap, m.is_complex != 0, m.compute_f32 != 0);
    ImputeSizes s{};
    s.N = m.N, s.K = r.K, s.T = m.T, s.cap = m.cap, s.zw = m.is_complex ? 2 : 1, s.esz = m.compute_f32 ? 4 : 8;
    s.maxm = p->maxm, s.ngrid = r.ngrid, s.welems = p->welems, s.cdf_inst = p->cdf_inst, s.nq = r.nq;
    s.u_trials = (p->sampling && !p->seeded) ? p->ntrial : 0;
    s.site_grid_doubles = r.grid_per_site() ? grid_doubles(m, true, r.ngrid) : 0;
    s.dist = r.dist;
    const ImputeBlock b = impute_plan_block(s, free_b, chunk_gb_override());
    if (b.nomem)
        return fail(c, MPST_ERR_NOMEM, "one instance needs %.3f GB of device scratch (%d environments, densities%s), %.3f GB are free: "
                    "not even a block of one instance fits", (double)b.per_bytes / (double)(1ull << 30), p->maxm,
                    p->cdf_inst ? ", cdf rows: raise cdf_stride" : "", (double)free_b / (double)(1ull << 30));
    p->chunk = b.chunk;
    return 0;
}

// the device side of a call: the caller's arrays, the scratch of a chunk, the results
struct ImputeBufs {
    DevBuf<uint8_t> miss, R, W;
    DevBuf<int32_t> ord;
    DevBuf<int64_t> row;
    DevBuf<double> gx, gp, u, p, S, x, e, lin, lev, q, cdf;
};

static int impute_upload(Ctx* c, const ImpModel& m, const ImputeRequest& r, const ImputePlan& p, ImputeBufs* b) {
    const int64_t N = m.N, K = r.K, chunk = p.chunk;
    const int T = m.T, zw = m.is_complex ? 2 : 1, ngrid = r.ngrid;
    const size_t esz = m.compute_f32 ? 4 : 8, nout = (size_t)N * K * T;
    const bool have_u = p.sampling && !p.seeded;
    int rc;
    if (r.nq > 0) {
        if ((rc = dalloc(c, b->lev, r.nq)) || (rc = dalloc(c, b->q, N * T * r.nq))) return rc;
        HIPC(c, hipMemcpy(b->lev, r.levels, (size_t)r.nq * sizeof(double), hipMemcpyHostToDevice));
        HIPC(c, hipMemset(b->q, 0, (size_t)N * T * r.nq * sizeof(double)));
    }
    if (p.cdf_inst > 0 && (rc = dalloc(c, b->cdf, chunk * p.cdf_inst))) return rc;
    if ((rc = dalloc(c, b->miss, N * T)) || (rc = dalloc(c, b->R, (int64_t)(chunk * p.maxm * m.cap * m.cap * zw * esz))) ||
        (rc = dalloc(c, b->gx, ngrid)) || (rc = dalloc(c, b->gp, grid_doubles(m, r.grid_per_site(), r.ngrid))) || (rc = dalloc(c, b->p, chunk * K * ngrid)) ||
        (rc = dalloc(c, b->S, chunk * K * ngrid)) || (rc = dalloc(c, b->x, N * K * T)) || (rc = dalloc(c, b->e, N * K * T))) return rc;
    if (have_u && (rc = dalloc(c, b->u, N * K * T * p.ntrial))) return rc;
    if (p.seeded && r.row_id) {
        if ((rc = dalloc(c, b->row, N))) return rc;
        HIPC(c, hipMemcpy(b->row, r.row_id, (size_t)N * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    if ((rc = dalloc(c, b->ord, N))) return rc;
    HIPC(c, hipMemcpy(b->ord, p.order.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
    if (p.welems && (rc = dalloc(c, b->W, (int64_t)(chunk * p.welems * esz)))) return rc;
    HIPC(c, hipMemcpy(b->miss, r.missing, (size_t)N * T, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(b->gx, r.grid_x, (size_t)ngrid * sizeof(double), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(b->gp, r.grid_phi, (size_t)grid_doubles(m, r.grid_per_site(), r.ngrid) * sizeof(double), hipMemcpyHostToDevice));
    if (have_u) HIPC(c, hipMemcpy(b->u, r.u, (size_t)N * K * T * p.ntrial * sizeof(double), hipMemcpyHostToDevice));
    HIPC(c, hipMemset(b->x, 0, nout * sizeof(double)));
    HIPC(c, hipMemset(b->e, 0, nout * sizeof(double)));
    return 0;
}

// closed form or table, decided from the grid the caller handed over (the Legendre table goes to the device); the kernels' arguments by name
static int impute_params(Ctx* c, const ImpModel& m, const ImputeRequest& r, const ImputePlan& p, ImputeBufs* b, ImputeParams* q) {
    std::vector<double> lin;
    ImpArgs& g = q->g;
    // (a per-site table is never looked at for a closed form: the call takes the table route, one instance per workgroup)
    q->trig = r.grid_per_site() ? 0
              : m.is_complex ? (fourier_grid(r.grid_x, (const double*)r.grid_phi, r.ngrid, m.d, &g.x0, &g.dxu) ? 1 : 0)
                             : (legendre_grid(r.grid_x, (const double*)r.grid_phi, r.ngrid, m.d, &g.x0, &g.dxu, &lin) ? 1 : 0);
    c->impute_trig = q->trig;
    if (!lin.empty()) {
        if (int rc = dalloc(c, b->lin, (int64_t)lin.size())) return rc;
        HIPC(c, hipMemcpy(b->lin, lin.data(), lin.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    q->work = b->W;
    q->order = b->ord;
    g.missing = b->miss;
    g.Rbuf = b->R;
    g.grid_x = b->gx;
    g.grid_phi = b->gp;
    g.grid_site_stride = r.grid_per_site() ? (int64_t)r.ngrid * m.d * (m.is_complex ? 2 : 1) : 0;
    g.u = b->u;
    g.pbuf = b->p;
    g.sbuf = b->S;
    g.x_out = b->x;
    g.err_out = b->e;
    g.max_missing = p.maxm;
    g.ngrid = r.ngrid;
    g.method = r.o->method;
    g.get_wmad = r.o->get_err;
    g.rev = r.o->order == MPST_IMPUTE_BACKWARDS ? 1 : 0;
    g.ntrial = p.ntrial;
    g.mean_basis = r.o->mean_basis;
    g.reject_thr = r.o->rejection_threshold;
    g.lin = b->lin;
    g.ntraj = (int)r.K;
    g.use_seed = p.seeded ? 1 : 0;
    g.seed = (unsigned long long)r.seed;
    g.row_id = b->row;
    g.levels = b->lev;
    g.q_out = b->q;
    g.cdf_out = b->cdf;
    g.nq = r.nq;
    g.cdf_stride = r.cdf_stride;
    g.cdf_rows = r.cdf_rows;
    g.ncdf = (int)p.ncdf;
    return 0;
}

// What an imputation call does around its blocks (run_blocks).  The kernels' arguments are worked out inside the timed span, as they
// always were.  The cdf rows of a block are staged in its slots and scattered to the caller's array after its sweep; the block then
// starts at an event of its own, so that neither the copy nor the clearing of the slots is in a phase.
struct ImputeHooks {
    Ctx* c; const ImpModel& m; const ImputeRequest& r; const ImputePlan& p;
    ImputeBufs* b; ImputeParams* q;
    std::vector<double> stage;          // the block's cdf rows on the host
    bool own_begin() const { return p.cdf_inst > 0; }
    int prepare() {
        stage.resize(p.cdf_inst > 0 ? (size_t)(p.chunk * p.cdf_inst) : 0);
        return impute_params(c, m, r, p, b, q);
    }
    int before(int64_t, int64_t) {      // rows beyond an instance's missing sites stay zero
        if (p.cdf_inst > 0) HIPC(c, hipMemsetAsync(q->g.cdf_out, 0, (size_t)(p.chunk * p.cdf_inst) * sizeof(double), c->stream));
        return 0;
    }
    int after(int64_t i0, int64_t cnt) {        // slot s of the block holds the rows of instance order[i0 + s]
        if (p.cdf_inst == 0) return 0;
        HIPC(c, hipMemcpyAsync(stage.data(), q->g.cdf_out, (size_t)(cnt * p.cdf_inst) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        for (int64_t sl = 0; sl < cnt; ++sl)
            memcpy(r.cdf_out + (size_t)p.order[i0 + sl] * p.cdf_inst, stage.data() + (size_t)sl * p.cdf_inst, (size_t)p.cdf_inst * sizeof(double));
        return 0;
    }
};

// shared tail of the imputation entry points: option checks, plan, scratch, launches, results.  One event between the two kernels of
// every block: the split of the pass into its environment and density halves (mpst_get_impute_phases) costs nothing against kernels
// of tens of milliseconds
static int run_impute(Ctx* c, const ImpModel& m, const ImputeRequest& r) {
    ImputePlan p;
    if (int rc = impute_validate(c, m, r, &p)) return rc;
    const int64_t N = m.N, T = m.T;
    if (r.nq > 0) memset(r.q_out, 0, (size_t)N * T * r.nq * sizeof(double));
    if (r.cdf_stride > 0) memset(r.cdf_out, 0, (size_t)N * r.cdf_rows * (size_t)p.ncdf * sizeof(double));
    std::vector<double> xo((size_t)N * r.K * T, 0.0), eo(xo.size(), 0.0);           // x_out / err_out: [N][K][T]
    c->impute_env_wgs = c->impute_chains = 0;
    p.order = impute_plan_order(r.missing, N, T, r.o->order == MPST_IMPUTE_BACKWARDS, getenv("MPST_IMP_NO_ORDER") != nullptr);
    if (p.maxm > 0) {
        size_t free_b = 0;
        ImputeBufs b;
        ImputeParams q{};
        int rc;
        if ((rc = free_device_bytes(c, &free_b)) || (rc = impute_block(c, m, r, free_b, &p)) || (rc = impute_upload(c, m, r, p, &b))) return rc;
        auto enqueue = [&](int64_t i0, int64_t cnt, hipEvent_t mid) {
            c->impute_batched = launch_impute(m, q, i0, cnt, c->stream, mid);
            if (c->impute_batched < 0) return fail(c, MPST_ERR_DEVICE, "no imputation kernel is built for this call's route");
            c->impute_env_wgs += (int)cnt;
            c->impute_chains += (int)(cnt * r.K);
            return 0;
        };
        if ((rc = run_blocks(c, N, p.chunk, true, r.seconds, enqueue, ImputeHooks{c, m, r, p, &b, &q, {}}))) return rc;
#ifdef MPST_LAB
        if (const char* e = getenv("MPST_IMB_DBG"); e && (atoi(e) & 8)) {   // phase clocks of the batched sweep (k_imp_leftb, workgroup 0 of the last block)
            double ph[6] = {0, 0, 0, 0, 0, 0};
            HIPC(c, hipMemcpy(ph, b.p, sizeof(ph), hipMemcpyDeviceToHost));
            fprintf(stderr, "[imb] phase A %.0f us, barrier %.0f, B1 %.0f, B2 %.0f, barrier %.0f\n", ph[0] * 0.01, ph[1] * 0.01, ph[2] * 0.01,
                    ph[3] * 0.01, ph[4] * 0.01);
        }
#endif
        HIPC(c, hipMemcpy(xo.data(), b.x, xo.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(eo.data(), b.e, eo.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (r.nq > 0) HIPC(c, hipMemcpy(r.q_out, b.q, (size_t)N * T * r.nq * sizeof(double), hipMemcpyDeviceToHost));
    } else if (r.seconds) {
        *r.seconds = 0.0;
    }
    memcpy(r.x_out, xo.data(), xo.size() * sizeof(double));
    if (r.err_out) memcpy(r.err_out, eo.data(), eo.size() * sizeof(double));
    return 0;
}

// The marginal likelihoods logp_out[N][C] of the instances under every class (mpst_marginal_model), on the imputation engine's buffers
// and route: no grid, no environments kept, one kernel per block of instances; missing may be NULL (nothing missing).
constexpr int MARGINAL_MAX_CLASSES = 16;
static int run_marginal(Ctx* c, const ImpModel& m, const uint8_t* missing, int C, double* logp_out, double* seconds) {
    const int64_t N = m.N;
    const int esz = m.compute_f32 ? 4 : 8;
    hipError_t ea = impute_init_attrs(c->device);
    if (ea != hipSuccess) return fail(c, MPST_ERR_DEVICE, "hipFuncSetAttribute failed: %s", hipGetErrorString(ea));
    const int64_t welems = marginal_work_elems(m.cap, m.is_complex != 0, m.compute_f32 != 0);
    size_t free_b = 0;
    int rc;
    if (welems && (rc = free_device_bytes(c, &free_b))) return rc;
    const int64_t chunk = marginal_plan_block(N, welems, esz, free_b);
    std::vector<int32_t> order((size_t)N);
    for (int64_t i = 0; i < N; ++i) order[i] = (int32_t)i;
    ImputeBufs b;
    ImputeParams q{};
    if ((rc = dalloc(c, b.ord, N)) || (rc = dalloc(c, b.x, N * C)) || (missing && (rc = dalloc(c, b.miss, N * m.T))) ||
        (welems && (rc = dalloc(c, b.W, (int64_t)(chunk * welems * esz))))) return rc;
    HIPC(c, hipMemcpy(b.ord, order.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
    if (missing) HIPC(c, hipMemcpy(b.miss, missing, (size_t)N * m.T, hipMemcpyHostToDevice));
    q.g.missing = b.miss;
    q.g.x_out = b.x;
    q.work = b.W;
    q.order = b.ord;
    q.nclass = C;
    rc = run_blocks(c, N, chunk, false, seconds, [&](int64_t i0, int64_t cnt, hipEvent_t) {
        if (launch_marginal(m, q, i0, cnt, c->stream) < 0) return fail(c, MPST_ERR_DEVICE, "the marginal-likelihood kernel did not launch: %s", hipGetErrorString(hipGetLastError()));
        return 0;
    });
    if (rc) return rc;
    HIPC(c, hipMemcpy(logp_out, b.x, (size_t)N * C * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// One mpst_site_conditionals call: the observed values x_obs[N][T], the grid, and the five outputs, each of which may be NULL
struct SitecondRequest {
    const mpst_sitecond_opts* o;
    const double *x_obs, *grid_x;
    const void* grid_phi;
    int32_t ngrid;
    double *nll_out, *pit_out, *med_out, *err_out, *q_out, *seconds;
};
// The leave-one-out site conditionals of a request: the walk's left rows and the amplitudes are the scratch of a block of instances
// (mpst_query_plan.h: sitecond_plan_block); the grid phase keeps ngrid doubles of density and prefix sums per workgroup, whatever the
// block.  The phases are the walk and the grid phase.
constexpr int SITECOND_MAX_CLASSES = 16;
static int run_sitecond(Ctx* c, const ImpModel& m, const SitecondRequest& r) {
    const int64_t N = m.N, T = m.T;
    const int zw = m.is_complex ? 2 : 1, nq = r.o->nq;
    const bool per_site = r.o->grid_per_site == 1;
    size_t free_b = 0;
    int rc;
    if ((rc = free_device_bytes(c, &free_b))) return rc;
    const SitecondBlock blk = sitecond_plan_block(N, m.T, m.cap, m.d, zw, free_b, chunk_gb_override());
    const int64_t chunk = blk.chunk;
    DevBuf<double> dx, gx, gp, lev, nll, pit, med, err, q, amp, lrows, pb, sb;
    if ((rc = dalloc(c, gx, r.ngrid)) || (rc = dalloc(c, gp, grid_doubles(m, per_site, r.ngrid))) || (rc = dalloc(c, amp, chunk * T * (m.d + 1) * zw)) ||
        (rc = dalloc(c, lrows, blk.tiles * T * SITECOND_TILE * m.cap * zw)) || (rc = dalloc(c, pb, blk.grid_wgs * r.ngrid)) ||
        (rc = dalloc(c, sb, blk.grid_wgs * r.ngrid)) ||
        (r.pit_out && (rc = dalloc(c, dx, N * T))) || (nq > 0 && ((rc = dalloc(c, lev, nq)) || (rc = dalloc(c, q, N * T * nq)))) ||
        (r.nll_out && (rc = dalloc(c, nll, N * T))) || (r.pit_out && (rc = dalloc(c, pit, N * T))) || (r.med_out && (rc = dalloc(c, med, N * T))) ||
        (r.err_out && (rc = dalloc(c, err, N * T)))) return rc;
    HIPC(c, hipMemcpy(gx, r.grid_x, (size_t)r.ngrid * sizeof(double), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(gp, r.grid_phi, (size_t)grid_doubles(m, per_site, r.ngrid) * sizeof(double), hipMemcpyHostToDevice));
    if (r.pit_out) HIPC(c, hipMemcpy(dx, r.x_obs, (size_t)(N * T) * sizeof(double), hipMemcpyHostToDevice));
    if (nq > 0) HIPC(c, hipMemcpy(lev, r.o->levels, (size_t)nq * sizeof(double), hipMemcpyHostToDevice));
    ScArgs g{};
    g.x = dx, g.grid_x = gx, g.grid_phi = gp, g.levels = lev;
    g.grid_site_stride = per_site ? (int64_t)r.ngrid * m.d * zw : 0;
    g.nll = nll, g.pit = pit, g.med = med, g.err = err, g.q = q;
    g.amp = amp, g.lrows = lrows, g.pbuf = pb, g.sbuf = sb;
    g.ngrid = r.ngrid, g.nq = nq, g.get_err = r.o->get_err ? 1 : 0;
    rc = run_blocks(c, N, chunk, true, r.seconds, [&](int64_t i0, int64_t cnt, hipEvent_t mid) {
        g.first = i0, g.count = cnt;
        if (launch_sitecond(m, g, c->stream, mid) < 0) return fail(c, MPST_ERR_DEVICE, "the site-conditional kernels did not launch: %s", hipGetErrorString(hipGetLastError()));
        return 0;
    });
    if (rc) return rc;
    const size_t nb = (size_t)(N * T) * sizeof(double);
    if (r.nll_out) HIPC(c, hipMemcpy(r.nll_out, nll, nb, hipMemcpyDeviceToHost));
    if (r.pit_out) HIPC(c, hipMemcpy(r.pit_out, pit, nb, hipMemcpyDeviceToHost));
    if (r.med_out) HIPC(c, hipMemcpy(r.med_out, med, nb, hipMemcpyDeviceToHost));
    if (r.err_out) HIPC(c, hipMemcpy(r.err_out, err, nb, hipMemcpyDeviceToHost));
    if (nq > 0) HIPC(c, hipMemcpy(r.q_out, q, nb * nq, hipMemcpyDeviceToHost));
    return 0;
}

// One mpst_window_conditionals call
struct WindowRequest {
    int32_t max_width;
    double *nll_out, *seconds;
};
// what a window call does around its blocks: a block's nll is its own on the device and goes to the caller's array after its kernels,
// outside the phases
struct WindowHooks {
    Ctx* c; const WindowRequest& r; double* dev_nll; int64_t per;     // per: doubles of one instance, T * max_width
    bool own_begin() const { return true; }
    int prepare() { return 0; }
    int before(int64_t, int64_t) { return 0; }
    int after(int64_t i0, int64_t cnt) {
        HIPC(c, hipMemcpyAsync(r.nll_out + (size_t)(i0 * per), dev_nll, (size_t)(cnt * per) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        return 0;
    }
};
// The window conditionals of a request: both rows of the walk and the block's nll are the scratch of a block of instances, the matrices
// of the window kernel's workgroups beyond the LDS limit come on top (mpst_query_plan.h: window_plan_block).  The phases are the walk
// and the window kernel.
constexpr int WINDOW_MAX_CLASSES = 16;
static int run_window(Ctx* c, const ImpModel& m, const WindowRequest& r) {
    const int64_t N = m.N, T = m.T;
    const int zw = m.is_complex ? 2 : 1;
    hipError_t ea = impute_init_attrs(c->device);
    if (ea != hipSuccess) return fail(c, MPST_ERR_DEVICE, "hipFuncSetAttribute failed: %s", hipGetErrorString(ea));
    size_t free_b = 0;
    int rc;
    if ((rc = free_device_bytes(c, &free_b))) return rc;
    const bool big = window_big_route(m.cap, m.is_complex != 0);
    const WindowBlock blk = window_plan_block(N, m.T, m.cap, zw, r.max_width, big, free_b, chunk_gb_override());
    DevBuf<double> rows, nll, work;
    if ((rc = dalloc(c, rows, blk.tiles * 2 * T * SITECOND_TILE * m.cap * zw)) || (rc = dalloc(c, nll, blk.chunk * T * r.max_width)) ||
        (big && (rc = dalloc(c, work, blk.win_wgs * WINDOW_BIG_MATS * m.cap * m.cap * zw)))) return rc;
    WinArgs g{};
    g.lrows = rows, g.nll = nll, g.work = work, g.max_width = r.max_width;
    return run_blocks(c, N, blk.chunk, true, r.seconds, [&](int64_t i0, int64_t cnt, hipEvent_t mid) {
        g.first = i0, g.count = cnt;
        const int64_t walk_wgs = (cnt + SITECOND_TILE - 1) / SITECOND_TILE, win_wgs = std::min<int64_t>(blk.win_wgs, cnt * T);
        if (launch_window(m, g, walk_wgs, win_wgs, c->stream, mid) < 0) return fail(c, MPST_ERR_DEVICE, "the window-conditional kernels did not launch: %s", hipGetErrorString(hipGetLastError()));
        return 0;
    }, WindowHooks{c, r, nll, T * r.max_width});
}

// One mpst_prefix_marginals call
struct PrefixRequest {
    int32_t C, label_site;
    double *logp_out, *seconds;
};
// what a prefix call does around its blocks: a block's results are its own on the device and go to the caller's array after its walk,
// outside the phases
struct PrefixHooks {
    Ctx* c; const PrefixRequest& r; double* dev_logp; int64_t per;      // per: doubles of one instance, (T + 1) * C
    bool own_begin() const { return true; }
    int prepare() { return 0; }
    int before(int64_t, int64_t) { return 0; }
    int after(int64_t i0, int64_t cnt) {
        HIPC(c, hipMemcpyAsync(r.logp_out + (size_t)(i0 * per), dev_logp, (size_t)(cnt * per) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        return 0;
    }
};
// The prefix marginals of a request: the G tables of the model live for the whole call and must fit the budget as they are, the class
// rows of the walk and the block's results are the scratch of a block of instances (mpst_prefix_plan.h: prefix_plan).  The phases are
// the environment kernel, which the first block launches ahead of its walk, and the walk with its scores.
constexpr int PREFIX_MAX_CLASSES = 16;
static int run_prefix(Ctx* c, const ImpModel& m, const PrefixRequest& r) {
    const int64_t N = m.N, T = m.T;
    const int zw = m.is_complex ? 2 : 1, Cn = r.C;
    hipError_t ea = impute_init_attrs(c->device);
    if (ea != hipSuccess) return fail(c, MPST_ERR_DEVICE, "hipFuncSetAttribute failed: %s", hipGetErrorString(ea));
    size_t free_b = 0;
    int rc;
    if ((rc = free_device_bytes(c, &free_b))) return rc;
    const bool big = prefix_big_route(m.cap, m.is_complex != 0);
    const PrefixPlan p = prefix_plan(N, m.T, Cn, r.label_site, m.cap, zw, big, free_b, chunk_gb_override());
    if (p.nomem)
        return fail(c, MPST_ERR_NOMEM, "the %lld environment tables of the model need %.3f GB of device memory, the budget of a query is %.3f GB: "
                    "they are not cut over the prefix length", (long long)p.mats, (double)p.table_bytes / (double)(1ull << 30),
                    query_budget(free_b, chunk_gb_override()) / (double)(1ull << 30));
    const int64_t mat = (int64_t)m.cap * m.cap * zw;
    DevBuf<double> G, lnG, work, crows, lp;
    if ((rc = dalloc(c, G, p.mats * mat)) || (rc = dalloc(c, lnG, (T + 1) * Cn)) || (big && (rc = dalloc(c, work, (int64_t)Cn * PREFIX_ENV_BIG_MATS * mat))) ||
        (rc = dalloc(c, crows, p.tiles * (Cn + 1) * PREFIX_TILE * m.cap * zw)) || (rc = dalloc(c, lp, p.chunk * (T + 1) * Cn))) return rc;
    PrefixArgs g{};
    g.G = G, g.lnG = lnG, g.work = work, g.crows = crows, g.logp = lp, g.C = Cn;
    bool tables = false;
    return run_blocks(c, N, p.chunk, true, r.seconds, [&](int64_t i0, int64_t cnt, hipEvent_t mid) {
        g.first = i0, g.count = cnt;
        if (!tables && launch_prefix_env(m, g, c->stream) < 0) return fail(c, MPST_ERR_DEVICE, "the prefix environment kernel did not launch: %s", hipGetErrorString(hipGetLastError()));
        tables = true;
        HIPC(c, hipEventRecord(mid, c->stream));
        if (launch_prefix_score(m, g, c->stream) < 0) return fail(c, MPST_ERR_DEVICE, "the prefix walk did not launch: %s", hipGetErrorString(hipGetLastError()));
        return 0;
    }, PrefixHooks{c, r, lp, (T + 1) * Cn});
}

// One mpst_segment_marginals call
struct SegmentRequest {
    int32_t C, label_site, max_width;
    double *logp_out, *lnorm_out, *seconds;
};
// what a segment call does around its blocks: a block's results are its own on the device and go to the caller's array after its walk,
// outside the phases
struct SegmentHooks {
    Ctx* c; double* host_logp; double* dev_logp; int64_t per;           // per: doubles of one instance, T * max_width * C
    bool own_begin() const { return true; }
    int prepare() { return 0; }
    int before(int64_t, int64_t) { return 0; }
    int after(int64_t i0, int64_t cnt) {
        HIPC(c, hipMemcpyAsync(host_logp + (size_t)(i0 * per), dev_logp, (size_t)(cnt * per) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        return 0;
    }
};
// The segment marginals of a request: the L and G tables of the model and the scratch of the walk's resident workgroups live for the
// whole call and must fit the budget as they are; a block of instances brings only its own results (mpst_segment_plan.h: segment_plan).
// The phases are the two table kernels, which the first block launches ahead of its walk, and the walk.  The context's launch figures
// (mpst_get_impute_info) become (0, 0, blocks of the walk, (series, start) items).
constexpr int SEGMENT_MAX_CLASSES = 16;
static int run_segment(Ctx* c, const ImpModel& m, const SegmentRequest& r) {
    const int64_t N = m.N, T = m.T;
    const int zw = m.is_complex ? 2 : 1, Cn = r.C;
    hipError_t ea = impute_init_attrs(c->device);
    if (ea != hipSuccess) return fail(c, MPST_ERR_DEVICE, "hipFuncSetAttribute failed: %s", hipGetErrorString(ea));
    size_t free_b = 0;
    int rc, cus = 0;
    if ((rc = free_device_bytes(c, &free_b))) return rc;
    HIPC(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const bool big = prefix_big_route(m.cap, m.is_complex != 0);
    const SegmentPlan p = segment_plan(N, m.T, Cn, r.label_site, m.cap, zw, r.max_width, big, cus, free_b, chunk_gb_override());
    if (p.nomem)
        return fail(c, MPST_ERR_NOMEM, "the %lld tables of the model and the walk's scratch need %.3f GB of device memory, the budget of a query is "
                    "%.3f GB: they are not cut", (long long)p.mats, (double)p.table_bytes / (double)(1ull << 30),
                    query_budget(free_b, chunk_gb_override()) / (double)(1ull << 30));
    const int64_t mat = (int64_t)m.cap * m.cap * zw;
    DevBuf<double> L, G, lnL, lnG, wl, wr, work, lp;
    if ((rc = dalloc(c, L, segment_left_mats(m.T, Cn, r.label_site) * mat)) || (rc = dalloc(c, G, prefix_table_mats(m.T, Cn, r.label_site) * mat)) ||
        (rc = dalloc(c, lnL, (T + 1) * Cn)) || (rc = dalloc(c, lnG, (T + 1) * Cn)) ||
        (big && ((rc = dalloc(c, wl, (int64_t)Cn * PREFIX_ENV_BIG_MATS * mat)) || (rc = dalloc(c, wr, (int64_t)Cn * PREFIX_ENV_BIG_MATS * mat)) ||
                 (rc = dalloc(c, work, p.walk_wgs * SEGMENT_BIG_MATS * mat)))) ||
        (rc = dalloc(c, lp, p.chunk * T * r.max_width * Cn))) return rc;
    SegmentArgs g{};
    g.L = L, g.lnL = lnL, g.G = G, g.lnG = lnG, g.work_left = wl, g.work_right = wr, g.work = work, g.logp = lp;
    g.C = Cn, g.max_width = r.max_width;
    int blocks = 0;
    rc = run_blocks(c, N, p.chunk, true, r.seconds, [&](int64_t i0, int64_t cnt, hipEvent_t mid) {
        g.first = i0, g.count = cnt;
        if (blocks == 0 && launch_segment_tables(m, g, c->stream) < 0) return fail(c, MPST_ERR_DEVICE, "the segment table kernels did not launch: %s", hipGetErrorString(hipGetLastError()));
        ++blocks;
        HIPC(c, hipEventRecord(mid, c->stream));
        if (launch_segment_walk(m, g, p.walk_wgs, c->stream) < 0) return fail(c, MPST_ERR_DEVICE, "the segment walk did not launch: %s", hipGetErrorString(hipGetLastError()));
        return 0;
    }, SegmentHooks{c, r.logp_out, lp, T * r.max_width * Cn});
    if (rc) return rc;
    c->impute_trig = c->impute_batched = 0;
    c->impute_env_wgs = blocks;
    c->impute_chains = (int)std::min<int64_t>(N * T, INT32_MAX);
    if (r.lnorm_out) HIPC(c, hipMemcpy(r.lnorm_out, lnG, (size_t)Cn * sizeof(double), hipMemcpyDeviceToHost));      // lnG[0][c] = ln ||W_c||^2
    return 0;
}

// One mpst_marginal_conditionals call: the mask and the values (either may be NULL), the grid, and the six outputs, each of which may be NULL
struct MargcondRequest {
    const mpst_sitecond_opts* o;
    const uint8_t* missing;
    const double *x, *grid_x;
    const void* grid_phi;
    int32_t ngrid;
    double *nll_out, *pit_out, *med_out, *err_out, *mean_out, *q_out, *seconds;
};
// what a marginal-conditionals call does around its blocks: a block's outputs are its own on the device and go to the caller's arrays
// after its kernels, outside the phases
struct MargcondHooks {
    Ctx* c; int64_t T; int nq;
    double* dev[6]; double* host[6];    // nll, pit, med, err, mean, q
    bool own_begin() const { return true; }
    int prepare() { return 0; }
    int before(int64_t, int64_t) { return 0; }
    int after(int64_t i0, int64_t cnt) {
        for (int k = 0; k < 6; ++k) {
            if (!host[k]) continue;
            const int64_t per = T * (k == 5 ? nq : 1);
            HIPC(c, hipMemcpyAsync(host[k] + (size_t)(i0 * per), dev[k], (size_t)(cnt * per) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        HIPC(c, hipStreamSynchronize(c->stream));
        return 0;
    }
};
// The marginal site conditionals of a request: the kept densities, rho_t and the outputs of a block of instances are its scratch, the
// walk's matrices beyond the LDS limit come on top (mpst_query_plan.h: margcond_plan_block); the grid phase keeps ngrid doubles of
// density and prefix sums per workgroup, whatever the block.  The phases are the walk and the grid phase.
constexpr int MARGCOND_MAX_CLASSES = 16;
static int run_margcond(Ctx* c, const ImpModel& m, const MargcondRequest& r) {
    const int64_t N = m.N, T = m.T;
    const int zw = m.is_complex ? 2 : 1, nq = r.o->nq;
    const bool per_site = r.o->grid_per_site == 1;
    hipError_t ea = impute_init_attrs(c->device);
    if (ea != hipSuccess) return fail(c, MPST_ERR_DEVICE, "hipFuncSetAttribute failed: %s", hipGetErrorString(ea));
    size_t free_b = 0;
    int rc;
    if ((rc = free_device_bytes(c, &free_b))) return rc;
    const bool big = margcond_big_route(m.cap, m.is_complex != 0);
    const int outputs = (r.nll_out ? 1 : 0) + (r.pit_out ? 1 : 0) + (r.med_out ? 1 : 0) + (r.err_out ? 1 : 0) + (r.mean_out ? 1 : 0) + nq;
    const MargcondBlock blk = margcond_plan_block(N, m.T, m.cap, m.d, zw, outputs, big, free_b, chunk_gb_override());
    const int64_t chunk = blk.chunk, mat = (int64_t)m.cap * m.cap * zw;
    DevBuf<double> dx, gx, gp, lev, nll, pit, med, err, mean, q, dens, rho, work, pb, sb;
    DevBuf<uint8_t> miss;
    if ((rc = dalloc(c, gx, r.ngrid)) || (rc = dalloc(c, gp, grid_doubles(m, per_site, r.ngrid))) || (rc = dalloc(c, dens, chunk * T * mat)) ||
        (rc = dalloc(c, rho, chunk * T * m.d * m.d * zw)) || (big && (rc = dalloc(c, work, chunk * MARGCOND_BIG_MATS * mat))) ||
        (rc = dalloc(c, pb, blk.grid_wgs * r.ngrid)) || (rc = dalloc(c, sb, blk.grid_wgs * r.ngrid)) ||
        (r.x && (rc = dalloc(c, dx, N * T))) || (r.missing && (rc = dalloc(c, miss, N * T))) ||
        (nq > 0 && ((rc = dalloc(c, lev, nq)) || (rc = dalloc(c, q, chunk * T * nq)))) ||
        (r.nll_out && (rc = dalloc(c, nll, chunk * T))) || (r.pit_out && (rc = dalloc(c, pit, chunk * T))) ||
        (r.med_out && (rc = dalloc(c, med, chunk * T))) || (r.err_out && (rc = dalloc(c, err, chunk * T))) ||
        (r.mean_out && (rc = dalloc(c, mean, chunk * T)))) return rc;
    HIPC(c, hipMemcpy(gx, r.grid_x, (size_t)r.ngrid * sizeof(double), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(gp, r.grid_phi, (size_t)grid_doubles(m, per_site, r.ngrid) * sizeof(double), hipMemcpyHostToDevice));
    if (r.x) HIPC(c, hipMemcpy(dx, r.x, (size_t)(N * T) * sizeof(double), hipMemcpyHostToDevice));
    if (r.missing) HIPC(c, hipMemcpy(miss, r.missing, (size_t)(N * T), hipMemcpyHostToDevice));
    if (nq > 0) HIPC(c, hipMemcpy(lev, r.o->levels, (size_t)nq * sizeof(double), hipMemcpyHostToDevice));
    McArgs g{};
    g.missing = miss, g.x = dx, g.grid_x = gx, g.grid_phi = gp, g.levels = lev;
    g.grid_site_stride = per_site ? (int64_t)r.ngrid * m.d * zw : 0;
    g.nll = nll, g.pit = pit, g.med = med, g.err = err, g.mean = mean, g.q = q;
    g.dens = dens, g.rho = rho, g.work = work, g.pbuf = pb, g.sbuf = sb;
    g.ngrid = r.ngrid, g.nq = nq, g.get_err = r.o->get_err ? 1 : 0;
    return run_blocks(c, N, chunk, true, r.seconds, [&](int64_t i0, int64_t cnt, hipEvent_t mid) {
        g.first = i0, g.count = cnt;
        if (launch_margcond(m, g, std::min<int64_t>(blk.grid_wgs, cnt * T), c->stream, mid) < 0)
            return fail(c, MPST_ERR_DEVICE, "the marginal-conditional kernels did not launch: %s", hipGetErrorString(hipGetLastError()));
        return 0;
    }, MargcondHooks{c, T, nq, {nll, pit, med, err, mean, q}, {r.nll_out, r.pit_out, r.med_out, r.err_out, r.mean_out, nq > 0 ? r.q_out : nullptr}});
}

// One mpst_observed_conditionals call: the kinds and parameters (validated by the entry point), the grid, and the outputs
struct ObservedRequest {
    const mpst_sitecond_opts* o;
    const uint8_t* kind;
    const double *a, *b;
    const void* E_user;
    const double *x, *grid_x;
    const void* grid_phi;
    int32_t ngrid;
    const mpst_observed_out* out;
    double* seconds;
};
// what an observed-conditionals call does around its blocks: the caller's operators of a block go to the device before its kernels, its
// outputs are its own on the device and go to the caller's arrays after them, both outside the phases
struct ObservedHooks {
    Ctx* c; int64_t T, op; int nq;          // op: doubles of one operator
    const double* E_user; double* devE;
    double* dev[12]; double* host[12];      // the ten per-site outputs (q: 3 and 7), logev, E_out
    bool own_begin() const { return true; }
    int prepare() { return 0; }
    int before(int64_t i0, int64_t cnt) {
        if (E_user) HIPC(c, hipMemcpyAsync(devE, E_user + (size_t)(i0 * T * op), (size_t)(cnt * T * op) * sizeof(double), hipMemcpyHostToDevice, c->stream));
        return 0;
    }
    int after(int64_t i0, int64_t cnt) {
        for (int k = 0; k < 12; ++k) {
            if (!host[k]) continue;
            const int64_t per = k == 10 ? 1 : k == 11 ? T * op : T * ((k == 3 || k == 7) ? nq : 1);
            HIPC(c, hipMemcpyAsync(host[k] + (size_t)(i0 * per), dev[k], (size_t)(cnt * per) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        HIPC(c, hipStreamSynchronize(c->stream));
        return 0;
    }
};
// The observed conditionals of a request: run_margcond's scratch plus the operators of a block (mpst_observed_plan.h:
// observed_plan_block).  The phases are (operators + walk, grid phase); the grid phase runs only if a per-site output is asked for.
static int run_observed(Ctx* c, const ImpModel& m, const ObservedRequest& r) {
    const int64_t N = m.N, T = m.T;
    const int zw = m.is_complex ? 2 : 1, nq = r.o->nq;
    const bool per_site = r.o->grid_per_site == 1;
    const mpst_observed_out& u = *r.out;
    hipError_t ea = impute_init_attrs(c->device);
    if (ea != hipSuccess) return fail(c, MPST_ERR_DEVICE, "hipFuncSetAttribute failed: %s", hipGetErrorString(ea));
    size_t free_b = 0;
    int rc;
    if ((rc = free_device_bytes(c, &free_b))) return rc;
    const bool big = margcond_big_route(m.cap, m.is_complex != 0);
    double* const site_out[10] = {u.pred_med, u.pred_err, u.pred_mean, nq > 0 ? u.pred_q : nullptr, u.post_med, u.post_err, u.post_mean,
                                  nq > 0 ? u.post_q : nullptr, u.nll_obs, u.pit};
    int outputs = 0;
    bool grid = false;
    for (int k = 0; k < 10; ++k)
        if (site_out[k]) outputs += (k == 3 || k == 7) ? nq : 1, grid = true;
    const ObservedBlock blk = observed_plan_block(N, m.T, m.cap, m.d, zw, outputs, big, free_b, chunk_gb_override());
    const int64_t chunk = blk.chunk, mat = (int64_t)m.cap * m.cap * zw, op = (int64_t)m.d * m.d * zw;
    const bool soft = r.a && r.b;
    DevBuf<double> dx, da, db, gx, gp, lev, so[10], logev, E, dens, rho, work, pb, sb;
    DevBuf<uint8_t> kind;
    if ((rc = dalloc(c, gx, r.ngrid)) || (rc = dalloc(c, gp, grid_doubles(m, per_site, r.ngrid))) || (rc = dalloc(c, dens, chunk * T * mat)) ||
        (rc = dalloc(c, rho, chunk * T * op)) || (rc = dalloc(c, E, chunk * T * op)) || (rc = dalloc(c, logev, chunk)) ||
        (big && (rc = dalloc(c, work, chunk * MARGCOND_BIG_MATS * mat))) ||
        (rc = dalloc(c, pb, blk.grid_wgs * r.ngrid)) || (rc = dalloc(c, sb, blk.grid_wgs * r.ngrid)) ||
        (r.x && (rc = dalloc(c, dx, N * T))) || (r.kind && (rc = dalloc(c, kind, N * T))) ||
        (soft && ((rc = dalloc(c, da, N * T)) || (rc = dalloc(c, db, N * T)))) || (nq > 0 && (rc = dalloc(c, lev, nq)))) return rc;
    for (int k = 0; k < 10; ++k)
        if (site_out[k] && (rc = dalloc(c, so[k], chunk * T * ((k == 3 || k == 7) ? nq : 1)))) return rc;
    HIPC(c, hipMemcpy(gx, r.grid_x, (size_t)r.ngrid * sizeof(double), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(gp, r.grid_phi, (size_t)grid_doubles(m, per_site, r.ngrid) * sizeof(double), hipMemcpyHostToDevice));
    if (r.x) HIPC(c, hipMemcpy(dx, r.x, (size_t)(N * T) * sizeof(double), hipMemcpyHostToDevice));
    if (r.kind) HIPC(c, hipMemcpy(kind, r.kind, (size_t)(N * T), hipMemcpyHostToDevice));
    if (soft) {
        HIPC(c, hipMemcpy(da, r.a, (size_t)(N * T) * sizeof(double), hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(db, r.b, (size_t)(N * T) * sizeof(double), hipMemcpyHostToDevice));
    }
    if (nq > 0) HIPC(c, hipMemcpy(lev, r.o->levels, (size_t)nq * sizeof(double), hipMemcpyHostToDevice));
    ObsArgs g{};
    g.kind = kind, g.a = da, g.b = db, g.x = dx, g.grid_x = gx, g.grid_phi = gp, g.levels = lev;
    g.grid_site_stride = per_site ? (int64_t)r.ngrid * m.d * zw : 0;
    g.pred_med = so[0], g.pred_err = so[1], g.pred_mean = so[2], g.pred_q = so[3];
    g.post_med = so[4], g.post_err = so[5], g.post_mean = so[6], g.post_q = so[7], g.nll = so[8], g.pit = so[9];
    g.logev = logev, g.E = E, g.dens = dens, g.rho = rho, g.work = work, g.pbuf = pb, g.sbuf = sb;
    g.ngrid = r.ngrid, g.nq = nq, g.get_err = r.o->get_err ? 1 : 0;
    ObservedHooks hooks{c, T, op, nq, (const double*)r.E_user, E, {}, {}};
    for (int k = 0; k < 10; ++k) hooks.dev[k] = so[k], hooks.host[k] = site_out[k];
    hooks.dev[10] = logev, hooks.host[10] = u.logev;
    hooks.dev[11] = E, hooks.host[11] = (double*)u.E_out;
    return run_blocks(c, N, chunk, true, r.seconds, [&](int64_t i0, int64_t cnt, hipEvent_t mid) {
        g.first = i0, g.count = cnt;
        if (launch_observed(m, g, std::min<int64_t>(blk.grid_wgs, cnt * T), grid, c->stream, mid) < 0)
            return fail(c, MPST_ERR_DEVICE, "the observed-conditional kernels did not launch: %s", hipGetErrorString(hipGetLastError()));
        return 0;
    }, hooks);
}

// One mpst_rolling_forecasts call: the horizons, the values (may be NULL), the grid, and the six outputs, each of which may be NULL
struct RollingRequest {
    const mpst_sitecond_opts* o;
    int32_t C, label_site, max_horizon;
    const double *x, *grid_x;
    const void* grid_phi;
    int32_t ngrid;
    double *nll_out, *pit_out, *med_out, *err_out, *mean_out, *q_out, *seconds;
};
// The rolling forecasts of a request (mpst_rolling_plan.h: rolling_plan).  G / lnG and the scratch of the table kernel live for the
// whole call and must fit the budget as they are; the chains are cut over blocks of targets, the series over blocks by what is left.  A
// block of series walks its rows, then takes the blocks of targets one after the other - the chains of a block of targets, then the score
// of every (origin, horizon) whose target lies in it - and finishes with the grid phase: with more than one block of series the chains
// are formed again for each.  The phases are (tables + rows + score, grid phase).
constexpr int ROLLING_MAX_CLASSES = 16;
static int run_rolling(Ctx* c, const ImpModel& m, const RollingRequest& r) {
    const int64_t N = m.N, T = m.T, H = r.max_horizon;
    const int zw = m.is_complex ? 2 : 1, nq = r.o->nq, Cn = r.C;
    const bool per_site = r.o->grid_per_site == 1;
    hipError_t ea = impute_init_attrs(c->device);
    if (ea != hipSuccess) return fail(c, MPST_ERR_DEVICE, "hipFuncSetAttribute failed: %s", hipGetErrorString(ea));
    size_t free_b = 0;
    int rc;
    if ((rc = free_device_bytes(c, &free_b))) return rc;
    const bool big = prefix_big_route(m.cap, m.is_complex != 0);
    const int outputs = (r.nll_out ? 1 : 0) + (r.pit_out ? 1 : 0) + (r.med_out ? 1 : 0) + (r.err_out ? 1 : 0) + (r.mean_out ? 1 : 0) + nq;
    const RollingPlan p = rolling_plan(N, m.T, Cn, r.label_site, m.cap, m.d, zw, r.max_horizon, outputs, big, free_b, chunk_gb_override());
    if (p.nomem)
        return fail(c, MPST_ERR_NOMEM, "the tables of the model and the table kernel's scratch need %.3f GB of device memory, the budget of a query is "
                    "%.3f GB: they are not cut", (double)p.fixed_bytes / (double)(1ull << 30),
                    query_budget(free_b, chunk_gb_override()) / (double)(1ull << 30));
    const int64_t chunk = p.chunk, mat = (int64_t)m.cap * m.cap * zw, trip = chunk * T * H;
    DevBuf<double> dx, gx, gp, lev, nll, pit, med, err, mean, q, G, lnG, wenv, K, work, rows, lrow, rho, pb, sb;
    if ((rc = dalloc(c, gx, r.ngrid)) || (rc = dalloc(c, gp, grid_doubles(m, per_site, r.ngrid))) ||
        (rc = dalloc(c, G, prefix_table_mats(m.T, Cn, r.label_site) * mat)) || (rc = dalloc(c, lnG, (T + 1) * Cn)) ||
        (big && (rc = dalloc(c, wenv, (int64_t)Cn * PREFIX_ENV_BIG_MATS * mat))) ||
        (rc = dalloc(c, K, p.tblock * rolling_target_mats(r.max_horizon, Cn, m.d) * mat)) || (rc = dalloc(c, work, p.table_wgs * mat)) ||
        (rc = dalloc(c, rows, chunk * T * Cn * m.cap * zw)) || (rc = dalloc(c, lrow, chunk * T * Cn)) ||
        (rc = dalloc(c, rho, trip * m.d * m.d * zw)) || (rc = dalloc(c, pb, p.grid_wgs * r.ngrid)) || (rc = dalloc(c, sb, p.grid_wgs * r.ngrid)) ||
        (r.x && (rc = dalloc(c, dx, N * T))) || (nq > 0 && ((rc = dalloc(c, lev, nq)) || (rc = dalloc(c, q, trip * nq)))) ||
        (r.nll_out && (rc = dalloc(c, nll, trip))) || (r.pit_out && (rc = dalloc(c, pit, trip))) || (r.med_out && (rc = dalloc(c, med, trip))) ||
        (r.err_out && (rc = dalloc(c, err, trip))) || (r.mean_out && (rc = dalloc(c, mean, trip)))) return rc;
    HIPC(c, hipMemcpy(gx, r.grid_x, (size_t)r.ngrid * sizeof(double), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(gp, r.grid_phi, (size_t)grid_doubles(m, per_site, r.ngrid) * sizeof(double), hipMemcpyHostToDevice));
    if (r.x) HIPC(c, hipMemcpy(dx, r.x, (size_t)(N * T) * sizeof(double), hipMemcpyHostToDevice));
    if (nq > 0) HIPC(c, hipMemcpy(lev, r.o->levels, (size_t)nq * sizeof(double), hipMemcpyHostToDevice));
    RollingArgs g{};
    g.x = dx, g.grid_x = gx, g.grid_phi = gp, g.levels = lev;
    g.grid_site_stride = per_site ? (int64_t)r.ngrid * m.d * zw : 0;
    g.nll = nll, g.pit = pit, g.med = med, g.err = err, g.mean = mean, g.q = q;
    g.G = G, g.lnG = lnG, g.K = K, g.work = work, g.rows = rows, g.lrow = lrow, g.rho = rho, g.pbuf = pb, g.sbuf = sb;
    g.C = Cn, g.H = r.max_horizon, g.ngrid = r.ngrid, g.nq = nq, g.get_err = r.o->get_err ? 1 : 0;
    int blocks = 0, tblocks = 0;
    rc = run_blocks(c, N, chunk, true, r.seconds, [&](int64_t i0, int64_t cnt, hipEvent_t mid) {
        g.first = i0, g.count = cnt;
        if (blocks == 0) {
            PrefixArgs e{};
            e.G = G, e.lnG = lnG, e.work = wenv, e.C = Cn;
            if (launch_prefix_env(m, e, c->stream) < 0) return fail(c, MPST_ERR_DEVICE, "the environment kernel did not launch: %s", hipGetErrorString(hipGetLastError()));
        }
        ++blocks;
        if (launch_rolling_rows(m, g, c->stream) < 0) return fail(c, MPST_ERR_DEVICE, "the rolling row kernel did not launch: %s", hipGetErrorString(hipGetLastError()));
        for (int64_t u0 = 0; u0 < T; u0 += p.tblock) {
            g.u0 = (int)u0, g.u1 = (int)std::min<int64_t>(T, u0 + p.tblock);
            if (blocks == 1) ++tblocks;
            if (launch_rolling_tables(m, g, p.table_wgs, c->stream) < 0)
                return fail(c, MPST_ERR_DEVICE, "the rolling table and score kernels did not launch: %s", hipGetErrorString(hipGetLastError()));
        }
        HIPC(c, hipEventRecord(mid, c->stream));
        if (launch_rolling_grid(m, g, std::min<int64_t>(p.grid_wgs, cnt * T * H), c->stream) < 0)
            return fail(c, MPST_ERR_DEVICE, "the rolling grid kernel did not launch: %s", hipGetErrorString(hipGetLastError()));
        return 0;
    }, MargcondHooks{c, T * H, nq, {nll, pit, med, err, mean, q}, {r.nll_out, r.pit_out, r.med_out, r.err_out, r.mean_out, nq > 0 ? r.q_out : nullptr}});
    if (rc) return rc;
    c->impute_trig = c->impute_batched = 0;
    c->impute_env_wgs = blocks;
    c->impute_chains = tblocks;
    return 0;
}

int mpst_get_impute_phases(void* ctx, double* seconds_out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !seconds_out) return MPST_ERR_INVALID;
    seconds_out[0] = c->impute_phase_s[0];
    seconds_out[1] = c->impute_phase_s[1];
    return 0;
}

int mpst_get_impute_info(void* ctx, int32_t* out, int32_t n) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !out || n < 0) return MPST_ERR_INVALID;
    const int32_t full[4] = {c->impute_trig, c->impute_batched, c->impute_env_wgs, c->impute_chains};
    for (int i = 0; i < n && i < 4; ++i) out[i] = full[i];
    return 0;
}

// K trajectories per instance: the argument checks the two *_traj entry points share
static int check_traj(Ctx* c, const mpst_impute_opts* o, int32_t K) {
    if (K < 1) return fail(c, MPST_ERR_INVALID, "num_trajectories must be at least 1 (got %d)", (int)K);
    if (o && o->method != MPST_IMPUTE_QUANTILE && o->method != MPST_IMPUTE_ITS_REJECT)
        return fail(c, MPST_ERR_UNSUPPORTED, "trajectories are drawn by the sampling methods (MPST_IMPUTE_QUANTILE, MPST_IMPUTE_ITS_REJECT): "
                                             "the median, mode and mean of an instance are one series");
    return 0;
}

// imputation on the model of a context's data set
static int impute_ctx(Ctx* c, int which, const ImputeRequest& r) {
    if (which != MPST_TRAIN && which != MPST_TEST) return fail(c, MPST_ERR_INVALID, "which must be 0 or 1");
    if (!c->have_mps || !c->have_opt) return fail(c, MPST_ERR_INVALID, "mpst_set_options / mpst_set_mps must be called first");
    const DataSet& s = c->ds[which];
    if (s.N <= 0) return fail(c, MPST_ERR_INVALID, "data set %d is empty", which);
    HIPC(c, hipSetDevice(c->device));
    const View v = make_view(c, which);
    const ImpModel m{v.sites, v.site_stride, v.chi, v.label_site, v.phi, v.label, s.N, c->T, c->d, c->mps.cap, c->zw == 2 ? 1 : 0,
                     (c->dtype == MPST_F32 || c->dtype == MPST_C64) ? 1 : 0};
    return run_impute(c, m, r);
}

int mpst_impute_dist(void* ctx, int which, const uint8_t* missing, const double* grid_x, const double* grid_phi, int32_t ngrid,
                     const mpst_impute_opts* o, double* x_out, double* err_out, double* seconds, int32_t nq, const double* levels,
                     double* q_out, int32_t cdf_stride, int32_t cdf_rows, double* cdf_out) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    return impute_ctx(c, which, impute_request(missing, grid_x, grid_phi, ngrid, o, nullptr, x_out, err_out, seconds)
                                    .dist_outputs(nq, levels, q_out, cdf_stride, cdf_rows, cdf_out));
}

int mpst_impute(void* ctx, int which, const uint8_t* missing, const double* grid_x, const double* grid_phi, int32_t ngrid,
                const mpst_impute_opts* o, const double* u, double* x_out, double* err_out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    return impute_ctx(c, which, impute_request(missing, grid_x, grid_phi, ngrid, o, u, x_out, err_out, seconds));
}

int mpst_impute_traj(void* ctx, int which, const uint8_t* missing, const double* grid_x, const double* grid_phi, int32_t ngrid,
                     const mpst_impute_opts* o, int32_t K, const double* u, int64_t seed, const int64_t* row_id, double* x_out,
                     double* err_out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (int rc = check_traj(c, o, K)) return rc;
    return impute_ctx(c, which, impute_request(missing, grid_x, grid_phi, ngrid, o, u, x_out, err_out, seconds).traj(K, seed, row_id));
}

// Host arrays of a model in the boundary layouts (site: (s, l, r[, c]) column-major like mpst_set_mps; phi: [N][T][d]) to
// the engine's layouts and element type.
extern "C++" {
template <typename R>
static void pack_model(const mpst_impute_model* h, int cap, int64_t stride, bool cx, std::vector<R>& sites, std::vector<R>& phi) {
    const int T = h->T, d = h->d, C = h->C, zw = cx ? 2 : 1;
    sites.assign((size_t)stride * T * zw, R(0));
    for (int j = 0; j < T; ++j) {
        const int Dl = h->chi[j], Dr = h->chi[j + 1], Cj = (j == h->label_site) ? C : 1;
        const double* src = (const double*)h->site[j];
        R* dst = &sites[(size_t)j * stride * zw];
        for (int cc = 0; cc < Cj; ++cc)
            for (int r = 0; r < Dr; ++r)
                for (int l = 0; l < Dl; ++l)
                    for (int s = 0; s < d; ++s) {
                        const size_t to = (((size_t)cc * Dl + l) * d + s) * Dr + r, from = s + (size_t)d * (l + (size_t)Dl * (r + (size_t)Dr * cc));
                        for (int z = 0; z < zw; ++z) dst[to * zw + z] = (R)src[from * zw + z];
                    }
    }
    const int64_t N = h->N;
    phi.resize((size_t)N * T * d * zw);
    const double* ps = (const double*)h->phi;
    for (int64_t i = 0; i < N; ++i)
        for (int j = 0; j < T; ++j)
            for (int s = 0; s < d * zw; ++s) phi[((size_t)j * N + i) * d * zw + s] = (R)ps[((size_t)i * T + j) * d * zw + s];
}
}  // extern "C++"

// The shape of a host model, for every entry point that takes one: pointers (phi and label_idx where the call reads them), sizes, the
// label site, the chain's ends, every bond dimension at least 1, every site tensor there.  *cap: the largest bond dimension.  What a
// call holds beyond that (element types, d, class and chi limits, labels in range) stays with the call.
static int check_model_shape(Ctx* c, const mpst_impute_model* h, bool need_phi, bool need_labels, int* cap) {
    if (!h || !h->site || !h->chi || (need_phi && !h->phi) || (need_labels && !h->label_idx)) return fail(c, MPST_ERR_INVALID, "NULL argument");
    if (h->T < 1 || h->d < 1 || h->C < 1 || (need_phi && h->N <= 0)) return fail(c, MPST_ERR_INVALID, "empty model or data");
    if (int rc = check_chain(c, h->chi, h->T, h->label_site, cap)) return rc;
    for (int j = 0; j < h->T; ++j)
        if (!h->site[j]) return fail(c, MPST_ERR_INVALID, "site[%d] is NULL", j);
    return 0;
}
// what the imputation engine's calls hold of a host model's element types and, where they read them, of its labels
static int check_model_types(Ctx* c, const mpst_impute_model* h, bool labels) {
    if (h->dtype != MPST_DTYPE_F64 && h->dtype != MPST_DTYPE_C64) return fail(c, MPST_ERR_INVALID, "dtype must be MPST_DTYPE_F64 or MPST_DTYPE_C64");
    if (h->compute != MPST_COMPUTE_F64 && h->compute != MPST_COMPUTE_F32) return fail(c, MPST_ERR_INVALID, "compute must be MPST_COMPUTE_F64 or MPST_COMPUTE_F32");
    for (int64_t i = 0; i < h->N && labels; ++i)
        if (h->label_idx[i] < 0 || h->label_idx[i] >= h->C) return fail(c, MPST_ERR_INVALID, "label_idx[%lld] out of range", (long long)i);
    return 0;
}

// A host model on the device for the length of a call: sites, phi, chi, label site and (where asked for) labels, and the view of them
// the engine reads.
struct DevModel {
    DevBuf<uint8_t> sites, phi;
    DevBuf<int32_t> chi, label_site, labels;
    ImpModel view{};
};
// packs a valid model (boundary layouts to the engine's, mpst_impute_model::compute as the element type) and uploads it
static int upload_model(Ctx* c, const mpst_impute_model* h, int cap, bool labels, DevModel* dm) {
    const bool cx = h->dtype == MPST_DTYPE_C64, f32 = h->compute == MPST_COMPUTE_F32;
    HIPC(c, hipSetDevice(c->device));
    const int64_t stride = (int64_t)h->C * cap * h->d * cap;
    const size_t esz = (f32 ? 4 : 8) * (cx ? 2 : 1);
    int rc;
    if ((rc = dalloc(c, dm->sites, (int64_t)(stride * h->T * esz))) || (rc = dalloc(c, dm->phi, (int64_t)(h->N * h->T * h->d * esz))) ||
        (rc = dalloc(c, dm->chi, h->T + 1)) || (rc = dalloc(c, dm->label_site, 1)) || (labels && (rc = dalloc(c, dm->labels, h->N)))) return rc;
    if (f32) {
        std::vector<float> hs, hp;
        pack_model<float>(h, cap, stride, cx, hs, hp);
        HIPC(c, hipMemcpy(dm->sites, hs.data(), hs.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(dm->phi, hp.data(), hp.size() * sizeof(float), hipMemcpyHostToDevice));
    } else {
        std::vector<double> hs, hp;
        pack_model<double>(h, cap, stride, cx, hs, hp);
        HIPC(c, hipMemcpy(dm->sites, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(dm->phi, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    HIPC(c, hipMemcpy(dm->chi, h->chi, (size_t)(h->T + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(dm->label_site, &h->label_site, sizeof(int32_t), hipMemcpyHostToDevice));
    if (labels) HIPC(c, hipMemcpy(dm->labels, h->label_idx, (size_t)h->N * sizeof(int32_t), hipMemcpyHostToDevice));
    dm->view = ImpModel{dm->sites, stride, dm->chi, dm->label_site, dm->phi, dm->labels, h->N, h->T, h->d, cap, cx ? 1 : 0, f32 ? 1 : 0};
    return 0;
}

// imputation on a model from host arrays
static int impute_host(Ctx* c, const mpst_impute_model* h, const ImputeRequest& r) {
    int cap = 0, rc;
    DevModel dm;
    if ((rc = check_model_shape(c, h, true, true, &cap)) || (rc = check_model_types(c, h, true)) || (rc = upload_model(c, h, cap, true, &dm))) return rc;
    return run_impute(c, dm.view, r);
}

int mpst_impute_model_dist(void* ctx, const mpst_impute_model* h, const uint8_t* missing, const double* grid_x, const void* grid_phi,
                           int32_t ngrid, const mpst_impute_opts* o, double* x_out, double* err_out, double* seconds, int32_t nq,
                           const double* levels, double* q_out, int32_t cdf_stride, int32_t cdf_rows, double* cdf_out) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    return impute_host(c, h, impute_request(missing, grid_x, grid_phi, ngrid, o, nullptr, x_out, err_out, seconds)
                                 .dist_outputs(nq, levels, q_out, cdf_stride, cdf_rows, cdf_out));
}

int mpst_impute_model_run(void* ctx, const mpst_impute_model* h, const uint8_t* missing, const double* grid_x, const void* grid_phi,
                          int32_t ngrid, const mpst_impute_opts* o, const double* u, double* x_out, double* err_out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    return impute_host(c, h, impute_request(missing, grid_x, grid_phi, ngrid, o, u, x_out, err_out, seconds));
}

int mpst_impute_model_traj(void* ctx, const mpst_impute_model* h, const uint8_t* missing, const double* grid_x, const void* grid_phi,
                           int32_t ngrid, const mpst_impute_opts* o, int32_t K, const double* u, int64_t seed, const int64_t* row_id,
                           double* x_out, double* err_out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (int rc = check_traj(c, o, K)) return rc;
    return impute_host(c, h, impute_request(missing, grid_x, grid_phi, ngrid, o, u, x_out, err_out, seconds).traj(K, seed, row_id));
}

int mpst_marginal_model(void* ctx, const mpst_impute_model* h, const uint8_t* missing, double* logp_out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (!h || !logp_out) return fail(c, MPST_ERR_INVALID, "NULL argument");
    int cap = 0, rc;
    if ((rc = check_model_shape(c, h, true, false, &cap))) return rc;
    if (h->d > 16 || h->C > MARGINAL_MAX_CLASSES)
        return fail(c, MPST_ERR_UNSUPPORTED, "marginal likelihoods hold d <= 16 and C <= %d (got %d, %d)", MARGINAL_MAX_CLASSES, h->d, h->C);
    if ((rc = check_model_types(c, h, false))) return rc;
    const int lim = impute_chi_limit(h->dtype == MPST_DTYPE_C64, h->compute == MPST_COMPUTE_F32);
    if (cap > lim) return fail(c, MPST_ERR_UNSUPPORTED, "marginal likelihoods hold chi_max <= %d (got %d)", lim, cap);
    DevModel dm;
    if ((rc = upload_model(c, h, cap, false, &dm))) return rc;
    return run_marginal(c, dm.view, missing, h->C, logp_out, seconds);
}

int mpst_site_conditionals(void* ctx, const mpst_impute_model* h, const double* x, const double* grid_x, const void* grid_phi, int32_t ngrid,
                           const mpst_sitecond_opts* o, double* nll_out, double* pit_out, double* med_out, double* err_out, double* q_out,
                           double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (!h || !x || !grid_x || !grid_phi || !o) return fail(c, MPST_ERR_INVALID, "NULL argument");
    if (!nll_out && !pit_out && !med_out && !err_out && !q_out) return fail(c, MPST_ERR_INVALID, "every output is NULL: nothing to compute");
    if (ngrid < 2) return fail(c, MPST_ERR_INVALID, "fewer than 2 grid values");
    int cap = 0, rc;
    if ((rc = check_grid_per_site(c, o->grid_per_site)) || (rc = check_levels(c, o->nq, o->levels, q_out))) return rc;
    if (!h->label_idx) return fail(c, MPST_ERR_INVALID, "label_idx is NULL: every series is conditioned under its own class");
    if ((rc = check_model_shape(c, h, true, true, &cap)) || (rc = check_model_types(c, h, true))) return rc;
    if (h->compute == MPST_COMPUTE_F32) return fail(c, MPST_ERR_UNSUPPORTED, "site conditionals run in fp64 only (compute = MPST_COMPUTE_F64)");
    if (cap > CAP_LIMIT || h->d > 16 || h->C > SITECOND_MAX_CLASSES)
        return fail(c, MPST_ERR_UNSUPPORTED, "site conditionals hold chi_max <= %d, d <= 16 and C <= %d (got %d, %d, %d)", CAP_LIMIT, SITECOND_MAX_CLASSES,
                    cap, h->d, h->C);
    DevModel dm;
    if ((rc = upload_model(c, h, cap, true, &dm))) return rc;
    return run_sitecond(c, dm.view, SitecondRequest{o, x, grid_x, grid_phi, ngrid, nll_out, pit_out, med_out, err_out, o->nq > 0 ? q_out : nullptr, seconds});
}

int mpst_window_conditionals(void* ctx, const mpst_impute_model* h, int32_t max_width, double* nll_out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (!h || !nll_out) return fail(c, MPST_ERR_INVALID, "NULL argument");
    if (!h->label_idx) return fail(c, MPST_ERR_INVALID, "label_idx is NULL: every series is conditioned under its own class");
    int cap = 0, rc;
    if ((rc = check_model_shape(c, h, true, true, &cap)) || (rc = check_model_types(c, h, true))) return rc;
    if (max_width < 1 || max_width > h->T) return fail(c, MPST_ERR_INVALID, "max_width must lie in 1 .. T = %d (got %d)", (int)h->T, (int)max_width);
    if (h->compute == MPST_COMPUTE_F32) return fail(c, MPST_ERR_UNSUPPORTED, "window conditionals run in fp64 only (compute = MPST_COMPUTE_F64)");
    if (cap > CAP_LIMIT || h->d > 16 || h->C > WINDOW_MAX_CLASSES)
        return fail(c, MPST_ERR_UNSUPPORTED, "window conditionals hold chi_max <= %d, d <= 16 and C <= %d (got %d, %d, %d)", CAP_LIMIT, WINDOW_MAX_CLASSES,
                    cap, h->d, h->C);
    DevModel dm;
    if ((rc = upload_model(c, h, cap, true, &dm))) return rc;
    return run_window(c, dm.view, WindowRequest{max_width, nll_out, seconds});
}

int mpst_marginal_conditionals(void* ctx, const mpst_impute_model* h, const uint8_t* missing, const double* x, const double* grid_x,
                               const void* grid_phi, int32_t ngrid, const mpst_sitecond_opts* o, double* nll_out, double* pit_out, double* med_out,
                               double* err_out, double* mean_out, double* q_out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (!h || !grid_x || !grid_phi || !o) return fail(c, MPST_ERR_INVALID, "NULL argument");
    if (!nll_out && !pit_out && !med_out && !err_out && !mean_out && !q_out) return fail(c, MPST_ERR_INVALID, "every output is NULL: nothing to compute");
    if (pit_out && !x) return fail(c, MPST_ERR_INVALID, "pit_out needs the values x");
    if (ngrid < 2) return fail(c, MPST_ERR_INVALID, "fewer than 2 grid values");
    int cap = 0, rc;
    if ((rc = check_grid_per_site(c, o->grid_per_site)) || (rc = check_levels(c, o->nq, o->levels, q_out))) return rc;
    if (!h->label_idx) return fail(c, MPST_ERR_INVALID, "label_idx is NULL: every series is conditioned under its own class");
    if ((rc = check_model_shape(c, h, true, true, &cap)) || (rc = check_model_types(c, h, true))) return rc;
    if (h->compute == MPST_COMPUTE_F32) return fail(c, MPST_ERR_UNSUPPORTED, "marginal conditionals run in fp64 only (compute = MPST_COMPUTE_F64)");
    if (cap > CAP_LIMIT || h->d > 16 || h->C > MARGCOND_MAX_CLASSES)
        return fail(c, MPST_ERR_UNSUPPORTED, "marginal conditionals hold chi_max <= %d, d <= 16 and C <= %d (got %d, %d, %d)", CAP_LIMIT,
                    MARGCOND_MAX_CLASSES, cap, h->d, h->C);
    DevModel dm;
    if ((rc = upload_model(c, h, cap, true, &dm))) return rc;
    return run_margcond(c, dm.view, MargcondRequest{o, missing, x, grid_x, grid_phi, ngrid, nll_out, pit_out, med_out, err_out, mean_out,
                                                    o->nq > 0 ? q_out : nullptr, seconds});
}

int mpst_observed_conditionals(void* ctx, const mpst_impute_model* h, const uint8_t* kind, const double* a, const double* b, const void* E_user,
                               const double* x, const double* grid_x, const void* grid_phi, int32_t ngrid, const mpst_sitecond_opts* o,
                               mpst_observed_out* out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (!h || !grid_x || !grid_phi || !o || !out) return fail(c, MPST_ERR_INVALID, "NULL argument");
    const bool any_q = out->pred_q || out->post_q;
    if (!out->pred_med && !out->pred_err && !out->pred_mean && !out->post_med && !out->post_err && !out->post_mean && !any_q && !out->nll_obs &&
        !out->pit && !out->logev && !out->E_out)
        return fail(c, MPST_ERR_INVALID, "every output is NULL: nothing to compute");
    if (out->pit && !x) return fail(c, MPST_ERR_INVALID, "pit needs the values x");
    if (ngrid < 2) return fail(c, MPST_ERR_INVALID, "fewer than 2 grid values");
    int cap = 0, rc;
    if ((rc = check_grid_per_site(c, o->grid_per_site)) || (rc = check_levels(c, o->nq, o->levels, out->pred_q ? out->pred_q : out->post_q))) return rc;
    if (!h->label_idx) return fail(c, MPST_ERR_INVALID, "label_idx is NULL: every series is conditioned under its own class");
    if ((rc = check_model_shape(c, h, true, true, &cap)) || (rc = check_model_types(c, h, true))) return rc;
    if (h->compute == MPST_COMPUTE_F32) return fail(c, MPST_ERR_UNSUPPORTED, "observed conditionals run in fp64 only (compute = MPST_COMPUTE_F64)");
    if (cap > CAP_LIMIT || h->d > 16 || h->C > MARGCOND_MAX_CLASSES)
        return fail(c, MPST_ERR_UNSUPPORTED, "observed conditionals hold chi_max <= %d, d <= 16 and C <= %d (got %d, %d, %d)", CAP_LIMIT,
                    MARGCOND_MAX_CLASSES, cap, h->d, h->C);
    if (kind) {
        const int64_t n = (int64_t)h->N * h->T;
        for (int64_t e = 0; e < n; ++e) {
            const long long i = (long long)(e / h->T);
            const int t = (int)(e % h->T), k = kind[e];
            if (k > MPST_OBS_OPERATOR) return fail(c, MPST_ERR_INVALID, "kind[%lld][%d] = %d is not one of MPST_OBS_* (0 .. 4)", i, t, k);
            if (k == MPST_OBS_OPERATOR && !E_user) return fail(c, MPST_ERR_INVALID, "kind[%lld][%d] is MPST_OBS_OPERATOR and E_user is NULL", i, t);
            if (k != MPST_OBS_GAUSS && k != MPST_OBS_INTERVAL) continue;
            if (!a || !b) return fail(c, MPST_ERR_INVALID, "kind[%lld][%d] = %d needs a and b", i, t, k);
            const bool fin = a[e] - a[e] == 0.0 && b[e] - b[e] == 0.0;
            if (k == MPST_OBS_GAUSS && !(fin && b[e] > 0.0))
                return fail(c, MPST_ERR_INVALID, "MPST_OBS_GAUSS at [%lld][%d]: a = %g must be finite and b = %g a positive finite number", i, t, a[e], b[e]);
            if (k == MPST_OBS_INTERVAL && !(fin && a[e] <= b[e]))
                return fail(c, MPST_ERR_INVALID, "MPST_OBS_INTERVAL at [%lld][%d]: the ends a = %g <= b = %g must be finite", i, t, a[e], b[e]);
        }
    }
    DevModel dm;
    if ((rc = upload_model(c, h, cap, true, &dm))) return rc;
    return run_observed(c, dm.view, ObservedRequest{o, kind, kind ? a : nullptr, kind ? b : nullptr, kind ? E_user : nullptr, x, grid_x, grid_phi,
                                                    ngrid, out, seconds});
}

int mpst_prefix_marginals(void* ctx, const mpst_impute_model* h, double* logp_out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (!h || !logp_out) return fail(c, MPST_ERR_INVALID, "NULL argument");
    int cap = 0, rc;
    if ((rc = check_model_shape(c, h, true, false, &cap))) return rc;
    if (h->compute != MPST_COMPUTE_F64) return fail(c, MPST_ERR_UNSUPPORTED, "prefix marginals run in fp64 only (compute = MPST_COMPUTE_F64)");
    if ((rc = check_model_types(c, h, false))) return rc;
    if (cap > CAP_LIMIT || h->d > 16 || h->C > PREFIX_MAX_CLASSES)
        return fail(c, MPST_ERR_UNSUPPORTED, "prefix marginals hold chi_max <= %d, d <= 16 and C <= %d (got %d, %d, %d)", CAP_LIMIT, PREFIX_MAX_CLASSES,
                    cap, h->d, h->C);
    DevModel dm;
    if ((rc = upload_model(c, h, cap, false, &dm))) return rc;
    return run_prefix(c, dm.view, PrefixRequest{h->C, h->label_site, logp_out, seconds});
}

int mpst_segment_marginals(void* ctx, const mpst_impute_model* h, int32_t max_width, double* logp_out, double* lnorm_out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (!h || !logp_out) return fail(c, MPST_ERR_INVALID, "NULL argument");
    int cap = 0, rc;
    if ((rc = check_model_shape(c, h, true, false, &cap))) return rc;
    if (max_width < 1 || max_width > h->T) return fail(c, MPST_ERR_INVALID, "max_width must lie in 1 .. T = %d (got %d)", (int)h->T, (int)max_width);
    if (h->compute != MPST_COMPUTE_F64) return fail(c, MPST_ERR_UNSUPPORTED, "segment marginals run in fp64 only (compute = MPST_COMPUTE_F64)");
    if ((rc = check_model_types(c, h, false))) return rc;
    if (cap > CAP_LIMIT || h->d > 16 || h->C > SEGMENT_MAX_CLASSES)
        return fail(c, MPST_ERR_UNSUPPORTED, "segment marginals hold chi_max <= %d, d <= 16 and C <= %d (got %d, %d, %d)", CAP_LIMIT, SEGMENT_MAX_CLASSES,
                    cap, h->d, h->C);
    DevModel dm;
    if ((rc = upload_model(c, h, cap, false, &dm))) return rc;
    return run_segment(c, dm.view, SegmentRequest{h->C, h->label_site, max_width, logp_out, lnorm_out, seconds});
}

int mpst_rolling_forecasts(void* ctx, const mpst_impute_model* h, int32_t max_horizon, const double* x, const double* grid_x, const void* grid_phi,
                           int32_t ngrid, const mpst_sitecond_opts* o, double* nll_out, double* pit_out, double* med_out, double* err_out,
                           double* mean_out, double* q_out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (!h || !grid_x || !grid_phi || !o) return fail(c, MPST_ERR_INVALID, "NULL argument");
    if (!nll_out && !pit_out && !med_out && !err_out && !mean_out && !q_out) return fail(c, MPST_ERR_INVALID, "every output is NULL: nothing to compute");
    if (pit_out && !x) return fail(c, MPST_ERR_INVALID, "pit_out needs the values x");
    if (ngrid < 2) return fail(c, MPST_ERR_INVALID, "fewer than 2 grid values");
    int cap = 0, rc;
    if ((rc = check_grid_per_site(c, o->grid_per_site)) || (rc = check_levels(c, o->nq, o->levels, q_out))) return rc;
    if (!h->label_idx) return fail(c, MPST_ERR_INVALID, "label_idx is NULL: every series is forecast under its own class, or under the mixture (-1)");
    if ((rc = check_model_shape(c, h, true, true, &cap)) || (rc = check_model_types(c, h, false))) return rc;
    for (int64_t i = 0; i < h->N; ++i)
        if (h->label_idx[i] < -1 || h->label_idx[i] >= h->C) return fail(c, MPST_ERR_INVALID, "label_idx[%lld] outside -1 .. C - 1", (long long)i);
    if (max_horizon < 1 || max_horizon > h->T) return fail(c, MPST_ERR_INVALID, "max_horizon must lie in 1 .. T = %d (got %d)", (int)h->T, (int)max_horizon);
    if (h->compute == MPST_COMPUTE_F32) return fail(c, MPST_ERR_UNSUPPORTED, "rolling forecasts run in fp64 only (compute = MPST_COMPUTE_F64)");
    if (cap > CAP_LIMIT || h->d > 16 || h->C > ROLLING_MAX_CLASSES)
        return fail(c, MPST_ERR_UNSUPPORTED, "rolling forecasts hold chi_max <= %d, d <= 16 and C <= %d (got %d, %d, %d)", CAP_LIMIT,
                    ROLLING_MAX_CLASSES, cap, h->d, h->C);
    DevModel dm;
    if ((rc = upload_model(c, h, cap, true, &dm))) return rc;
    return run_rolling(c, dm.view, RollingRequest{o, h->C, h->label_site, max_horizon, x, grid_x, grid_phi, ngrid, nll_out, pit_out, med_out, err_out,
                                                  mean_out, o->nq > 0 ? q_out : nullptr, seconds});
}

// ---- entanglement analysis (mpst_analysis.hip) ----------------------------------------------------------------------------
static int analysis_model(Ctx* c, const mpst_impute_model* h, bool need_phi, AnalysisHost* out) {
    int cap = 0;
    if (int rc = check_model_shape(c, h, need_phi, false, &cap)) return rc;
    if (h->dtype == MPST_DTYPE_C64)
        return fail(c, MPST_ERR_UNSUPPORTED, "entanglement analysis of a complex model: the reference computes it in Float64 only");
    if (h->dtype != MPST_DTYPE_F64) return fail(c, MPST_ERR_INVALID, "dtype must be MPST_DTYPE_F64");
    if (h->compute != MPST_COMPUTE_F64) return fail(c, MPST_ERR_UNSUPPORTED, "entanglement analysis runs in fp64 only (compute = MPST_COMPUTE_F64)");
    if (h->d > 16) return fail(c, MPST_ERR_UNSUPPORTED, "d = %d > 16", h->d);
    for (int j = 0; j <= h->T; ++j)
        if (h->chi[j] > 128) return fail(c, MPST_ERR_UNSUPPORTED, "chi[%d] = %d > 128", j, h->chi[j]);
    *out = AnalysisHost{h->T, h->d, h->C, h->label_site, h->chi, (const double* const*)h->site};
    return 0;
}

static int analysis_domain(Ctx* c, const AnalysisDomain& dm) {
    if (dm.kind == 1)
        return fail(c, MPST_ERR_DOMAIN, "RDM contains large negative eigenvalues outside of the tolerance 1.4901161193847656e-8: "
                    "lambda = %.17g (class %d, instance %lld, k %d, site %d)", dm.value, dm.cls, (long long)dm.inst, dm.k, dm.site);
    return fail(c, MPST_ERR_DOMAIN, "Tr(rho_corrected) > 1.0! (%.17g) (class %d, instance %lld, k %d, site %d)", dm.value, dm.cls,
                (long long)dm.inst, dm.k, dm.site);
}

int mpst_entanglement(void* ctx, const mpst_impute_model* m, double* bee_out, double* see_out) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    AnalysisHost h;
    int rc = analysis_model(c, m, false, &h);
    if (rc) return rc;
    HIPC(c, hipSetDevice(c->device));
    AnalysisDomain dm{};
    HIPC(c, analysis_entanglement(h, c->stream, bee_out, see_out, &dm));
    return dm.kind ? analysis_domain(c, dm) : 0;
}

int mpst_see_variation(void* ctx, const mpst_impute_model* m, int32_t cls, double* out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    AnalysisHost h;
    int rc = analysis_model(c, m, true, &h);
    if (rc) return rc;
    if (!out) return fail(c, MPST_ERR_INVALID, "NULL argument");
    if (cls < 0 || cls >= m->C) return fail(c, MPST_ERR_INVALID, "class %d out of range [0, %d)", cls, m->C);
    HIPC(c, hipSetDevice(c->device));
    AnalysisDomain dm{};
    HIPC(c, analysis_see_variation(h, cls, (const double*)m->phi, m->N, c->stream, out, seconds, &dm));
    return dm.kind ? analysis_domain(c, dm) : 0;
}

int mpst_pair_analysis(void* ctx, const mpst_impute_model* m, const double* obs, int32_t obs_per_site, double* mi_out, double* mean_out,
                       double* cov_out, double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    AnalysisHost h;
    if (int rc = analysis_model(c, m, false, &h)) return rc;
    if (!mi_out && !mean_out && !cov_out) return fail(c, MPST_ERR_INVALID, "every output is NULL: nothing to compute");
    if ((mean_out || cov_out) && !obs) return fail(c, MPST_ERR_INVALID, "mean_out and cov_out need an observable (obs is NULL)");
    if (obs_per_site != 0 && obs_per_site != 1)
        return fail(c, MPST_ERR_INVALID, "obs_per_site must be 0 (obs[d][d]) or 1 (obs[T][d][d]), got %d", (int)obs_per_site);
    if (mi_out && m->d > 11)
        return fail(c, MPST_ERR_UNSUPPORTED, "mutual information holds d <= 11 (the pair matrix is d^2 x d^2, the Jacobi n <= 128; got d = %d); "
                    "the moments have no such limit (mi_out = NULL)", m->d);
    HIPC(c, hipSetDevice(c->device));
    size_t free_b = 0;
    if (int rc = free_device_bytes(c, &free_b)) return rc;
    double ph[2] = {0.0, 0.0};
    HIPC(c, analysis_pairs(h, obs, obs_per_site != 0, free_b, chunk_gb_override(), c->stream, mi_out, mean_out, cov_out, seconds, ph));
    c->impute_phase_s[0] = ph[0];
    c->impute_phase_s[1] = ph[1];
    return 0;
}

// ---- model overlaps (mpst_overlap.hip) ------------------------------------------------------------------------------------
int mpst_model_overlaps(void* ctx, const mpst_impute_model* models, int32_t K, const int32_t* pairs, int32_t P, double* g_out, double* lg_out,
                        double* seconds) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (!models || !g_out || !lg_out) return fail(c, MPST_ERR_INVALID, "NULL argument");
    if (K < 1) return fail(c, MPST_ERR_INVALID, "K = %d: at least one model", (int)K);
    if (pairs && P < 0) return fail(c, MPST_ERR_INVALID, "P = %d is negative", (int)P);
    const mpst_impute_model& m0 = models[0];
    OverlapHost h{K, m0.T, m0.d, m0.label_site, m0.dtype == MPST_DTYPE_C64, {}, {}, {}, {}};
    for (int k = 0; k < K; ++k) {
        const mpst_impute_model* m = models + k;
        int cap = 0, rc;
        if ((rc = check_model_shape(c, m, false, false, &cap)) || (rc = check_model_types(c, m, false))) return rc;
        if (m->T != m0.T || m->d != m0.d || m->label_site != m0.label_site || m->dtype != m0.dtype)
            return fail(c, MPST_ERR_INVALID, "model %d disagrees with model 0 in T, d, label site or element type (%d, %d, %d, %d against %d, %d, %d, %d)", k,
                        m->T, m->d, m->label_site, m->dtype, m0.T, m0.d, m0.label_site, m0.dtype);
        if (m->compute != MPST_COMPUTE_F64) return fail(c, MPST_ERR_UNSUPPORTED, "model overlaps run in fp64 only (compute = MPST_COMPUTE_F64)");
        if (cap > CAP_LIMIT || m->d > 16 || m->d * cap > 1024 || m->C > 16)
            return fail(c, MPST_ERR_UNSUPPORTED, "model overlaps hold chi_max <= %d, d <= 16, d chi_max <= 1024 and C <= 16 (model %d: %d, %d, %d)", CAP_LIMIT,
                        k, cap, m->d, m->C);
        h.chi.push_back(m->chi);
        h.site.push_back(m->site);
        h.ncls.push_back(m->C);
    }
    if (pairs) {
        for (int64_t q = 0; q < 2ll * P; ++q)
            if (pairs[q] < 0 || pairs[q] >= K) return fail(c, MPST_ERR_INVALID, "pairs[%lld][%d] = %d outside [0, %d)", (long long)(q / 2), (int)(q % 2), pairs[q], (int)K);
        h.pairs.assign(pairs, pairs + 2ll * P);
    } else {
        for (int a = 0; a < K; ++a)
            for (int b = a; b < K; ++b) {
                h.pairs.push_back(a);
                h.pairs.push_back(b);
            }
    }
    HIPC(c, hipSetDevice(c->device));
    size_t free_b = 0;
    if (int rc = free_device_bytes(c, &free_b)) return rc;
    HIPC(c, model_overlaps(h, free_b, chunk_gb_override(), c->stream, g_out, lg_out, seconds));
    return 0;
}

int mpst_normalize(void* ctx) {
    Ctx* c = (Ctx*)ctx;
    int rc = check_ready(c);
    if (rc) return rc;
    View v = make_view(c, MPST_TRAIN);
    if (c->typed) {
        TView t = make_tview(c, MPST_TRAIN);
        launch_tnorm2(t, c->ws.norm2, c->ws.tnorm_scratch, c->stream);
        launch_tscale_sites(t, c->ws.norm2, c->stream);
    } else {
        launch_norm2(v, c->ws.norm2, c->ws.norm_scratch, c->stream);
        launch_scale_sites(v, c->ws.norm2, c->stream);
    }
    c->ynext_lid = -1;
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    return 0;
}

int mpst_set_profile(void* ctx, uint32_t kernel_mask) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    c->prof_mask = kernel_mask;
    c->epoch++;
    for (int i = 0; i < 16; ++i) { c->prof_us[i] = 0; c->prof_cnt[i] = 0; }
    return 0;
}

int mpst_get_profile(void* ctx, double* total_us, int64_t* count) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    for (int i = 0; i < 16; ++i) {
        if (total_us) total_us[i] = c->prof_us[i];
        if (count) count[i] = c->prof_cnt[i];
    }
    return 0;
}

int mpst_get_info(void* ctx, int32_t* out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !out) return MPST_ERR_INVALID;
    int rc = check_ready(c);
    if (rc) return rc;
    const int pk = c->opt.loss == MPST_LOSS_MSE ? 1 : 0;
    out[0] = c->ws.fused ? 1 : 0;
    out[1] = c->ws.big ? 1 : 0;
    out[2] = c->ds[MPST_TRAIN].nparts[pk];
    out[3] = c->ds[MPST_TRAIN].nchunks;
    out[4] = c->mps.cap;
    out[5] = c->nranks;
    out[6] = sweep_uses_graph(c) ? 1 : 0;
    out[7] = (int32_t)std::min<int64_t>(c->big_fallbacks, 1 << 30);
    out[8] = blocked_eig_coop_aborts(c->ws.blk);      // bonds the persistent tridiagonalisation handed back to the launch-per-step path
    out[9] = blocked_eig_xcd_misplaced(c->ws.blk);    // bonds whose XCD-local attempt found its workgroups on several XCDs (redone across the XCDs)
    out[10] = c->ws.b2 ? 1 : 0;                        // fused chain with the sliced bond GEMMs (k_yhat_s + k_grad_s)
    out[11] = c->ws.b2 ? c->ws.b2_ksplit : 0;             // shares per gradient block of k_grad_s
    out[12] = (!c->ws.big && eig_merged()) ? 1 : 0;    // tridiagonalisation + eigenvectors in one launch (k_eig_trivec)
    out[13] = c->big_redos;                          // large-bond sweeps redone bond by bond after a failed verdict
    out[14] = (c->ws.big_opt && !multi(c)) ? 1 : 0;                   // large bonds: the eigensolver's verdict is read once per sweep
    out[15] = c->typed ? 1 + c->dtype : 0;        // element-typed kernels in use: 1 + dtype
    return 0;
}

int mpst_get_info_n(void* ctx, int32_t* out, int32_t n) {
    int32_t full[23];
    if (!out || n < 0) return MPST_ERR_INVALID;
    int rc = mpst_get_info(ctx, full);
    if (rc) return rc;
    {
        Ctx* c4 = (Ctx*)ctx;
        View v4 = make_view(c4, MPST_TRAIN);
        // [18] the bonds of a sweep run the four-launch chain (k_bond_tail); [19] sweeps / bond steps whose tail was redone on the six-launch chain
        full[18] = bond_uses_tail(c4, v4, c4->opt.track_cost != 0) ? 1 : 0;
        full[19] = c4->tail_redos;
        // [20] on that chain, the S tile and the overlap product of the tail come from side workgroups of the k_eig_trivec launch (0: MPST_TAIL_PRE=0)
        full[20] = (full[18] && c4->ws.tail_pre) ? 1 : 0;
        // [21] with rebuild_caches, the side workgroups also rebuild the caches, a row per bond (0: MPST_REBUILD_SIDE=0, or any of the above off);
        // [22] rows they rebuilt in the last sweep: 2 max(0, T - 3) where [21], 0 elsewhere
        full[21] = rebuild_side_on(c4, v4) ? 1 : 0;
        full[22] = c4->rebuild_steps;
    }
    // bonds the subspace eigensolver attempted / whose result was accepted (the rest went to the exact solver), as of the last sweep,
    // batch or bond step that returned: cached at their synchronisation point, the query itself never waits for the stream
    full[16] = ((Ctx*)ctx)->ss_counts[0];
    full[17] = ((Ctx*)ctx)->ss_counts[1];
    for (int i = 0; i < n && i < 23; ++i) out[i] = full[i];
    return 0;
}

int mpst_get_eig_phases(void* ctx, double* us) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !c->ws.sc || !us) return MPST_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    DevScalars sc;
    HIPC(c, hipMemcpy(&sc, c->ws.sc, sizeof sc, hipMemcpyDeviceToHost));
    const unsigned long long* t = sc.eig_stamps;              // 100 MHz ticks
    us[0] = 0.01 * (double)(t[1] - t[0]);                     // k_eig_tri: tridiagonalisation
    us[1] = 0.01 * (double)(t[3] - t[2]);                     // k_eig_vec block 0: staging + bisection
    us[2] = 0.01 * (double)(t[4] - t[3]);                     //                    twisted factorisation
    us[3] = 0.01 * (double)(t[5] - t[4]);                     //                    back-transformation
    us[4] = 0.01 * (double)(t[9] - t[8]);                     // k_eig_fin: truncation, verification, Loewdin
    us[5] = (double)(t[7] - t[6]);                            // shader cycles spent in the tridiagonalisation
    return 0;
}

// phase stamps of the last stamped k_bond_tail launch (us since workgroup 0 started; -1: not taken): us[0..15] workgroup 0 (which also
// hosts a job of the next bond's tensor when the sweep goes on), us[16..31] the last workgroup (no role), us[32..35] the side workgroups
// of the bond's k_eig_trivec launch (see include/mpstime_hip.h)
int mpst_get_tail_phases(void* ctx, double* us) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !c->ws.sc || !us) return MPST_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    DevScalars sc;
    HIPC(c, hipMemcpy(&sc, c->ws.sc, sizeof sc, hipMemcpyDeviceToHost));
    const unsigned long long* t = sc.eig_stamps;
    const double t0 = (double)t[16];
    // workgroup 0: slots 16..31; the last workgroup: 32..47
    for (int i = 0; i < 48; ++i) us[i] = -1.0;
    for (int i = 0; i < 16; ++i) if (t[16 + i] && t[16]) us[i] = 0.01 * ((double)t[16 + i] - t0);
    for (int i = 0; i < 16; ++i) if (t[32 + i] && t[16]) us[16 + i] = 0.01 * ((double)t[32 + i] - t0);
    // slots a launch did not reach keep the stamps of an earlier one: nothing after the first stamp that runs backwards counts
    for (int g = 0; g < 2; ++g)
        for (int i = 1; i < 16; ++i)
            if (us[16 * g + i] < us[16 * g + i - 1] || us[16 * g + i - 1] == -1.0) us[16 * g + i] = -1.0;
    for (int i = 0; i < 4; ++i) us[48 + i] = (double)t[56 + i];        // bonds by |Z^T Z - I| of their candidates: < 1e-13, < 1e-8, < 3e-5, above
    // every workgroup of the stamped launch left (start, end) in the gradient workspace: earliest start, latest end, latest start
    us[52] = us[53] = us[54] = 0.0;
    {
        const size_t ng = (size_t)std::min<unsigned long long>(t[60], 2048ull);
        if (ng > 0 && c->ws.tail_span) {
            std::vector<unsigned long long> sp(2 * ng);
            HIPC(c, hipMemcpy(sp.data(), c->ws.tail_span, sp.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            unsigned long long s0 = ~0ull, s1 = 0ull, e1 = 0ull;
            for (size_t i = 0; i < ng; ++i) {
                s0 = std::min(s0, sp[2 * i]);
                s1 = std::max(s1, sp[2 * i]);
                e1 = std::max(e1, sp[2 * i + 1]);
            }
            us[52] = 0.01 * ((double)s0 - t0);
            us[53] = 0.01 * ((double)e1 - t0);
            us[54] = 0.01 * ((double)s1 - t0);
        }
    }
    // the side workgroups of that bond's k_eig_trivec launch (the launch BEFORE the tail: negative times): how many left a (start, end),
    // earliest start, latest start, latest end
    us[32] = us[33] = us[34] = us[35] = 0.0;
    {
        const size_t ns = (size_t)std::min<unsigned long long>(t[61], (unsigned long long)TS_SPAN);
        if (ns > 0 && c->ws.tail_span && c->ws.tail_pre && t[16]) {
            std::vector<unsigned long long> sp(2 * ns);
            HIPC(c, hipMemcpy(sp.data(), c->ws.tail_span + 2 * TS_SPAN, sp.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            unsigned long long s0 = ~0ull, s1 = 0ull, e1 = 0ull;
            for (size_t i = 0; i < ns; ++i) {
                s0 = std::min(s0, sp[2 * i]);
                s1 = std::max(s1, sp[2 * i]);
                e1 = std::max(e1, sp[2 * i + 1]);
            }
            us[32] = (double)ns;
            us[33] = 0.01 * ((double)s0 - t0);
            us[34] = 0.01 * ((double)s1 - t0);
            us[35] = 0.01 * ((double)e1 - t0);
        }
    }
    return 0;
}

#ifdef MPST_B2_DEBUG
// bring-up builds only (scratch/build_dbg.sh): stamps of the sliced bond kernels, 8192 x 8 slots
int mpst_debug_b2(void* ctx, unsigned long long* out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !c->ws.b2_dbg || !out) return MPST_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(out, c->ws.b2_dbg, 8192 * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

#endif

#ifdef MPST_TRI_DEBUG
// bring-up builds only (-DMPST_TRI_DEBUG): raw stamp slots of the eigensolver kernels
int mpst_debug_stamps(void* ctx, unsigned long long* out64) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !c->ws.sc || !out64) return MPST_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    DevScalars sc;
    HIPC(c, hipMemcpy(&sc, c->ws.sc, sizeof sc, hipMemcpyDeviceToHost));
    for (int i = 0; i < 64; ++i) out64[i] = sc.eig_stamps[i];
    return 0;
}
#endif

int mpst_selftest_mfma(void* ctx, const double* A, const double* B, int32_t K, double* C_out) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    DevBuf<double> dA, dB, dC;
    int rc;
    if ((rc = dalloc(c, dA, 16 * K)) || (rc = dalloc(c, dB, 16 * K)) || (rc = dalloc(c, dC, 256))) return rc;
    HIPC(c, hipMemcpy(dA, A, (size_t)16 * K * sizeof(double), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(dB, B, (size_t)16 * K * sizeof(double), hipMemcpyHostToDevice));
    launch_selftest_mfma(dA, dB, K, dC, c->stream);
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpy(C_out, dC, 256 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int mpst_selftest_eig(void* ctx, const double* G, int32_t n, int32_t alg, double* lambda_out, double* E_out, int32_t* sweeps) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return MPST_ERR_INVALID;
    if (n < 1 || n > DIM_LIMIT) return fail(c, MPST_ERR_INVALID, "n must be in 1..%d", DIM_LIMIT);
    if (alg < 0 || (alg & ~63)) return fail(c, MPST_ERR_INVALID, "alg %d: only bits 0..5 have a meaning", alg);
    if (n > MAX_DIM && (alg & (8 | 16)))
        return fail(c, MPST_ERR_INVALID, "alg bits 3 and 4 (64 eigenpairs, gated launcher) belong to the n <= %d solver, n = %d", MAX_DIM, n);
    if ((alg & 32) && !(alg & 16)) return fail(c, MPST_ERR_INVALID, "alg bit 5 (closed gate) needs bit 4 (gated launcher)");
    if ((alg & 16) && (alg & 7))
        return fail(c, MPST_ERR_INVALID, "alg bit 4: the gated launcher has one algorithm (tridiagonal, 64 eigenpairs), bits 0-2 must be 0");
    const bool gated = (alg & 16) != 0, gate_open = !(alg & 32);
    HIPC(c, hipSetDevice(c->device));
    DevBuf<double> dG, dl, dE, dws;
    DevBuf<int32_t> ds, dgate;
    hipError_t ea = eig_init_attrs(c->device);
    if (ea != hipSuccess) return fail(c, MPST_ERR_DEVICE, "hipFuncSetAttribute failed: %s", hipGetErrorString(ea));
    int rc;
    if ((rc = dalloc(c, dG, n * n)) || (rc = dalloc(c, dl, n)) || (rc = dalloc(c, dE, n * n)) || (rc = dalloc(c, ds, 1)) ||
        (rc = dalloc(c, dws, (int64_t)eig_workspace_doubles()))) return rc;
    HIPC(c, hipMemcpy(dG, G, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
    HIPC(c, hipMemset(dws, 0, eig_workspace_doubles() * sizeof(double)));
    if (n > MAX_DIM) {
        // alg 0: the hand-written blocked solver, library only if its verification asks for it; alg 2: the library alone
        std::string e;
        int need_lib = 1;
        View vraw{};
        vraw.zw = (alg & 4) ? 2 : 0;          // bit 2: G is the real embedding of a Hermitian matrix (one vector per eigenvalue pair)
        alg &= 3;
        if (alg != 2) {
            BlockedEig* bl = nullptr;
            if ((rc = blocked_eig_create(&bl, n, &e))) return fail(c, rc, "large-bond eigensolver: %s", e.c_str());
            HIPC(c, hipMemsetAsync(dl, 0, (size_t)n * sizeof(double), c->stream));
            HIPC(c, hipMemsetAsync(dE, 0, (size_t)n * n * sizeof(double), c->stream));
            need_lib = launch_eig_blocked(vraw, 0, 0, dG, n, dl, dE, ds, bl, c->stream);
            blocked_eig_destroy(bl);
            if (need_lib < 0) return fail(c, MPST_ERR_DEVICE, "blocked eigensolver failed");
        }
        if (need_lib && alg != 3) {
            BigEig* be = nullptr;
            if ((rc = big_eig_create(&be, n, c->stream, &e))) return fail(c, rc, "large-bond eigensolver: %s", e.c_str());
            rc = launch_eig_big_raw(dG, n, dl, dE, ds, be, c->stream);
            (void)hipStreamSynchronize(c->stream);
            big_eig_destroy(be);
            if (rc) return fail(c, rc, "the large-bond Jacobi solver could not be launched");
        }
    } else if (gated) {
        // the gated launcher clears nothing: zeros under an open gate, the sentinel under a closed one (which must come back untouched)
        constexpr double SENTINEL = -7.0;        // documented in mpstime_hip.h
        const double fill = gate_open ? 0.0 : SENTINEL;
        const int32_t gate = gate_open ? 1 : 0, info0 = gate_open ? 0 : (int32_t)SENTINEL;
        std::vector<double> hfill((size_t)n * n, fill);
        if ((rc = dalloc(c, dgate, 1))) return rc;
        HIPC(c, hipMemcpy(dl, hfill.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(dE, hfill.data(), (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(ds, &info0, sizeof info0, hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(dgate, &gate, sizeof gate, hipMemcpyHostToDevice));
        launch_eig_raw_gated(dG, n, dl, dE, ds, dws, dgate, c->stream);
    } else {
        launch_eig_raw(dG, n, alg, dl, dE, ds, dws, c->stream);
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpy(lambda_out, dl, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(E_out, dE, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost));
    if (sweeps) HIPC(c, hipMemcpy(sweeps, ds, sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
