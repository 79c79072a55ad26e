// dgp_api.hip -- the C ABI declared in include/dgp_hip.h: plan bookkeeping and stage sequencing.
#include <mutex>
#include <new>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>

#include "../../include/dgp_hip.h"
#include "dgp_common.h"
#include "dgp_internal.h"

using namespace dgp;

static thread_local char g_err[256] = "";
static int fail(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}
static int hipfail(hipError_t e, const char* where) {
  snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
  return (int)e;
}

// Small host -> device uploads (site sizes, the hyperparameters of large batches) go through PINNED staging slots that
// the plan owns: an asynchronous copy from pageable memory is only safe while the runtime happens to stage it before
// returning.  A slot is reused after the event recorded behind its last copy has completed.
struct PinnedRing {
  static constexpr int SLOTS = 4;
  void* buf[SLOTS];
  size_t cap[SLOTS];
  hipEvent_t ev[SLOTS];
  int busy[SLOTS], have_ev[SLOTS], next;
  void* acquire(size_t bytes) {
    const int i = next;
    if (busy[i]) {
      (void)hipEventSynchronize(ev[i]);
      busy[i] = 0;
    }
    if (cap[i] < bytes) {
      if (buf[i]) (void)hipHostFree(buf[i]);
      buf[i] = nullptr;
      cap[i] = 0;
      if (hipHostMalloc(&buf[i], bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
      cap[i] = bytes;
    }
    return buf[i];
  }
  void commit(hipStream_t s) {  // after the copy out of the slot handed out last has been enqueued on s
    const int i = next;
    if (!have_ev[i]) have_ev[i] = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
    if (have_ev[i] && hipEventRecord(ev[i], s) == hipSuccess) busy[i] = 1;
    else (void)hipStreamSynchronize(s);
    next = (next + 1) % SLOTS;
  }
  void destroy() {
    for (int i = 0; i < SLOTS; ++i) {
      if (busy[i]) (void)hipEventSynchronize(ev[i]);
      if (have_ev[i]) (void)hipEventDestroy(ev[i]);
      if (buf[i]) (void)hipHostFree(buf[i]);
    }
  }
};

struct dgp_plan {
  int model, dtype, d, ntheta;
  PinnedRing ring;
  int* nsite_host;        // host copy of the sites' sizes (B > 1): the inference entry points walk the sites on the host
  int B;                  // sites carried in lockstep (1 = plain plan); site b's buffers sit b * site_bytes further on
  size_t site_bytes;
  void* pre;              // device scratch for the batch's hyperparameters (B > 8), after the last site
  void* pre2;             // a second one for the fp64 evaluator of the refinement (fp32 plans), so that `pre` stays valid
  int pre_ready;          // the Gram build of the current step has uploaded them
  Tuning tune;            // tile-shape selectors (dgp_plan_set_option)
  int refine;             // fp32 plans: one step of iterative refinement with an fp64 residual after the solves
  int* nsite;             // device: the sites' own sizes (B > 1), after the hyperparameter scratch
  const void* dr_w;       // caller's [2][n] weight vectors for the out[DGP_OUT_DR_W0..] reductions, or null
  int64_t n, N;
  size_t elem;
  char* ws;
  size_t ws_bytes;
  // carved workspace
  void *Xt, *A, *Tm, *S, *z, *alpha, *gpart, *spart, *scal, *snap;
  int* info;
  hipStream_t sc;         // rest of the split panel chain (dgp_chol.hip::potrf_split)
  int lookahead, early;   // potrf schedule; issue the inverse's level recursion behind the factorisation's checkpoints
  int have_inputs, have_factor, have_inverse;
  hipStream_t s2, s3;     // bulk trailing updates; early inverse work
  hipEvent_t xev[8];      // checkpoints of the factorisation and fork/join events for s3
  int have_xev;
  hipEvent_t* ev;
  int nev;
  // optional HIP-event timing of the fit-step stages
  int timing, n_syrk, timed_valid;
  double syrk_flop;
  hipEvent_t* tev;   // 2 per stage (start, stop)
  hipEvent_t* sev;   // 2 per bulk syrk launch
  int nsev;
};
enum { TS_GRAM = 0, TS_POTRF, TS_TRTRI, TS_LAUUM, TS_SOLVE, TS_GRAD, TS_COUNT };

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct Layout {
  size_t Xt, A, Tm, S, z, alpha, gpart, spart, scal, info, snap, total;
};
static Layout layout(const dgp_plan* p) {
  Layout L;
  const size_t e = p->elem, N = (size_t)p->N;
  size_t o = 0;
  L.Xt = o; o += align_up(e * N * p->d);
  L.A = o; o += align_up(e * N * N);
  L.Tm = o; o += align_up(e * N * N);
  L.S = o; o += align_up(e * N * N);
  L.z = o; o += align_up(e * N);
  L.alpha = o; o += align_up(e * N);
  L.gpart = o; o += align_up(e * (size_t)gram_grad_partials(p->N));
  L.spart = o; o += align_up(e * (size_t)solve_partials(p->N));
  L.scal = o; o += align_up(e * 16);
  L.info = o; o += align_up(sizeof(int) * POTRF_INFO_INTS);
  L.snap = o; o += align_up(e * 2 * DGP_TILE_HOST * DGP_TILE_HOST);  // the split chain's two snapshot blocks
  L.total = o;
  return L;
}

static int default_lookahead() { return 2; }  // lookahead on: the group-ahead schedule of dgp_chol.hip::potrf
// panels per group of that schedule: pairs for one site (chain-bound), larger groups (K = 512 bulk updates) for a batch
// One site: pairs while the factorisation is chain-bound; from ~96 block columns on it is bound by its bulk updates, which
// gain from a longer K per read-modify-write pass over the trailing matrix (measured, one site: n = 16384 fp32 43.1 -> 42.1 ms
// per fit step with groups of 4, fp64 79.2 -> 77.2; n = 65536 fp32 2305 -> 2239 (4) -> 2216 ms (8); n = 8192: 12.44 -> 12.50
// with 4).  Batched plans: 4, 6 and 8 give the same factorisation time (n = 8192 x 32: 101.7 / 101.9 / 102.5 ms).
// Batched fp64 plans of 32 sites or more run these groups LEFT-LOOKING (dgp_chol.hip::potrf_scheduled, potrf_schedule_auto): each group
// of 4 columns is updated once, with everything to its left, instead of every trailing tile once per group at K = 512.
static int group_size(int lookahead, int batch, long nbk) {
  if (!lookahead) return 0;
  if (const char* e = getenv("DGP_GROUP")) return atoi(e) < 2 ? 2 : atoi(e);
  if (batch >= 4) return 4;
  return nbk >= 256 ? 8 : (nbk >= 96 ? 4 : 2);
}

// workgroups the EARLY inverse launches may occupy (one per CU): they share the GPU with the panel chain
#define EARLY_WG_CAP 384
// compute units those launches leave to the panel chain
#define EARLY_RESERVED_CUS 64

extern "C" {

int dgp_version(void) { return 1; }
const char* dgp_last_error(void) { return g_err; }
int dgp_model_ntheta(int model, int d) { return model_ntheta(model, d); }
int dgp_composite_define(const int* spec, int nspec, int* model_out) {
  if (!spec || nspec < 2 || !model_out) return fail(DGP_E_ARG, "dgp_composite_define: null argument");
  const int id = composite_define(spec, nspec);
  if (id == -5) return fail(DGP_E_FULL, "dgp_composite_define: the registry is full (64 distinct kernel structures per process)");
  if (id < 0) return fail(DGP_E_MODEL, "dgp_composite_define: malformed or unsupported kernel description");
  *model_out = id;
  return 0;
}
int64_t dgp_padded_n(int64_t n) { return round_up(n, DGP_TILE_HOST); }

int dgp_plan_create(int model, int dtype, int64_t n, int d, dgp_plan** out) {
  if (!out || n <= 0 || n > (1 << 20)) return fail(DGP_E_ARG, "dgp_plan_create: bad n / null out");
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_plan_create: dtype must be 0 (f64) or 1 (f32)");
  const int nt = model_ntheta(model, d);
  if (nt < 0) return fail(DGP_E_MODEL, "dgp_plan_create: unsupported (model, d)");
  dgp_plan* p = new (std::nothrow) dgp_plan();
  if (!p) return fail(DGP_E_ARG, "dgp_plan_create: out of host memory");
  memset(p, 0, sizeof(*p));
  p->model = model;
  p->dtype = dtype;
  p->d = d;
  p->ntheta = nt;
  p->n = n;
  p->N = round_up(n, DGP_TILE_HOST);
  p->elem = dtype == DGP_F64 ? 8 : 4;
  p->B = 1;
  p->lookahead = default_lookahead();
  p->early = getenv("DGP_NO_EARLY_TRTRI") ? 0 : 1;
  p->tune = default_tuning();
  p->refine = (dtype == DGP_F32 && !(getenv("DGP_NO_REFINE") && atoi(getenv("DGP_NO_REFINE")))) ? 1 : 0;
  *out = p;
  return 0;
}

int dgp_plan_destroy(dgp_plan* p) {
  if (!p) return 0;
  if (p->ev) {
    for (int i = 0; i < p->nev; ++i) (void)hipEventDestroy(p->ev[i]);
    delete[] p->ev;
  }
  if (p->tev) {
    for (int i = 0; i < 2 * TS_COUNT; ++i) (void)hipEventDestroy(p->tev[i]);
    delete[] p->tev;
  }
  if (p->sev) {
    for (int i = 0; i < p->nsev; ++i) (void)hipEventDestroy(p->sev[i]);
    delete[] p->sev;
  }
  // s2 / sc / s3 belong to the caller-stream's StreamSet (process lifetime), not to the plan
  if (p->have_xev)
    for (int i = 0; i < 8; ++i) (void)hipEventDestroy(p->xev[i]);
  p->ring.destroy();
  delete[] p->nsite_host;
  delete p;
  return 0;
}

size_t dgp_plan_workspace_bytes(const dgp_plan* p) {
  return p ? layout(p).total * (size_t)p->B + 2 * align_up(pre_scratch_bytes(p->B)) + (p->B > 1 ? align_up(sizeof(int) * p->B) : 0)
           : 0;
}

int dgp_plan_set_batch(dgp_plan* p, int batch) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (batch < 1 || batch > DGP_MAX_BATCH_SITES) return fail(DGP_E_ARG, "dgp_plan_set_batch: batch must be 1..1024");
  if (p->ws) return fail(DGP_E_STATE, "dgp_plan_set_batch: call before dgp_plan_set_workspace");
  p->B = batch;
  return 0;
}
int dgp_plan_batch(const dgp_plan* p) { return p ? p->B : 0; }

int dgp_plan_set_site_sizes(dgp_plan* p, const int64_t* sizes, void* stream) {
  if (!p || !sizes) return fail(DGP_E_ARG, "dgp_plan_set_site_sizes: null argument");
  if (!p->ws) return fail(DGP_E_WORKSPACE, "plan has no workspace: call dgp_plan_set_workspace");
  if (p->B == 1) {
    if (sizes[0] != p->n) return fail(DGP_E_ARG, "dgp_plan_set_site_sizes: an unbatched plan has the size it was created with");
    return 0;
  }
  for (int b = 0; b < p->B; ++b)
    if (sizes[b] < 1 || sizes[b] > p->n) return fail(DGP_E_ARG, "dgp_plan_set_site_sizes: sizes must be in 1..n");
  int* v = (int*)p->ring.acquire(sizeof(int) * (size_t)p->B);
  if (!v) return fail(DGP_E_ARG, "dgp_plan_set_site_sizes: out of pinned host memory");
  for (int b = 0; b < p->B; ++b) p->nsite_host[b] = v[b] = (int)sizes[b];
  hipError_t e = hipMemcpyAsync(p->nsite, v, sizeof(int) * (size_t)p->B, hipMemcpyHostToDevice, (hipStream_t)stream);
  p->ring.commit((hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "dgp_plan_set_site_sizes");
  p->have_factor = 0;
  return 0;
}

int dgp_plan_set_dr_weights(dgp_plan* p, const void* w_dev) {
  if (!p) return fail(DGP_E_ARG, "dgp_plan_set_dr_weights: null plan");
  p->dr_w = w_dev;
  return 0;
}

int dgp_plan_set_workspace(dgp_plan* p, void* dev_ptr, size_t bytes) {
  if (!p || !dev_ptr) return fail(DGP_E_ARG, "dgp_plan_set_workspace: null");
  const Layout L = layout(p);
  if (bytes < dgp_plan_workspace_bytes(p))
    return fail(DGP_E_WORKSPACE, "dgp_plan_set_workspace: workspace too small");
  p->site_bytes = L.total;
  if (((uintptr_t)dev_ptr & 255) != 0) return fail(DGP_E_ARG, "dgp_plan_set_workspace: pointer must be 256-byte aligned");
  p->ws = (char*)dev_ptr;
  p->ws_bytes = bytes;
  p->Xt = p->ws + L.Xt;
  p->A = p->ws + L.A;
  p->Tm = p->ws + L.Tm;
  p->S = p->ws + L.S;
  p->z = p->ws + L.z;
  p->alpha = p->ws + L.alpha;
  p->gpart = p->ws + L.gpart;
  p->spart = p->ws + L.spart;
  p->scal = p->ws + L.scal;
  p->info = (int*)(p->ws + L.info);
  p->snap = p->ws + L.snap;
  p->pre = pre_scratch_bytes(p->B) ? (void*)(p->ws + L.total * (size_t)p->B) : nullptr;
  p->pre2 = p->pre ? (void*)((char*)p->pre + align_up(pre_scratch_bytes(p->B))) : nullptr;
  p->nsite = nullptr;
  p->dr_w = nullptr;
  if (p->B > 1) {  // every site starts at the full size n
    p->nsite = (int*)(p->ws + L.total * (size_t)p->B + 2 * align_up(pre_scratch_bytes(p->B)));
    delete[] p->nsite_host;
    p->nsite_host = new (std::nothrow) int[(size_t)p->B];
    if (!p->nsite_host) return fail(DGP_E_ARG, "dgp_plan_set_workspace: out of host memory");
    for (int b = 0; b < p->B; ++b) p->nsite_host[b] = (int)p->n;
    hipError_t e = hipMemcpy(p->nsite, p->nsite_host, sizeof(int) * (size_t)p->B, hipMemcpyHostToDevice);  // blocking
    if (e != hipSuccess) return hipfail(e, "dgp_plan_set_workspace: hipMemcpy");
  }
  p->have_inputs = p->have_factor = 0;
  return 0;
}

int dgp_plan_set_option(dgp_plan* p, int key, int64_t value) {
  if (!p) return fail(DGP_E_ARG, "dgp_plan_set_option: null plan");
  switch (key) {
    case DGP_OPT_LAUUM64_MAX_TILES:
      if (value < 0 || value > (1 << 30)) return fail(DGP_E_ARG, "dgp_plan_set_option: value out of range");
      p->tune.lauum64_max_tiles = (int)value;
      return 0;
    case DGP_OPT_SYRK_SLOTS:
      if (value < 1 || value > (1 << 20)) return fail(DGP_E_ARG, "dgp_plan_set_option: value out of range");
      p->tune.syrk_slots = (int)value;
      return 0;
    case DGP_OPT_TRTRI_SMALL:
      if (value < 0) return fail(DGP_E_ARG, "dgp_plan_set_option: value out of range");
      p->tune.trtri_small = (long)value;
      return 0;
    case DGP_OPT_SYRK_ORDER:
    case DGP_OPT_LAUUM_ORDER:
      if (value < 0 || value > 64) return fail(DGP_E_ARG, "dgp_plan_set_option: value out of range");
      (key == DGP_OPT_SYRK_ORDER ? p->tune.syrk_super : p->tune.lauum_super) = (int)value;
      return 0;
    case DGP_OPT_CHAIN_YIELD:
      p->tune.chain_yield = value ? 1 : 0;
      return 0;
    case DGP_OPT_FUSED_GRAD:
      p->tune.fused_grad = value ? 1 : 0;
      return 0;
    case DGP_OPT_GROUP_GEMM:
      p->tune.group_gemm = value ? 1 : 0;
      return 0;
    case DGP_OPT_POTRF_SCHEDULE:
      if (value < 0 || value > 1) return fail(DGP_E_ARG, "dgp_plan_set_option: value out of range");
      p->tune.potrf_schedule = (int)value;
      return 0;
    case DGP_OPT_POTRF_SWEEP:
    case DGP_OPT_POTRF_TAIL:
    case DGP_OPT_POTRF_TAIL_SWEEP:
      if (value < 0 || value > (1 << 20)) return fail(DGP_E_ARG, "dgp_plan_set_option: value out of range");
      (key == DGP_OPT_POTRF_SWEEP ? p->tune.potrf_sweep : key == DGP_OPT_POTRF_TAIL ? p->tune.potrf_tail : p->tune.potrf_tail_sweep) = (int)value;
      return 0;
    case DGP_OPT_POTRF_SOLVE:
      p->tune.potrf_solve = value ? 1 : 0;
      return 0;
    case DGP_OPT_POTRF_OVERLAP:
      p->tune.potrf_overlap = value ? 1 : 0;
      return 0;
    case DGP_OPT_POTRF_SLOTS:
      if (value < 1 || value > (1 << 20)) return fail(DGP_E_ARG, "dgp_plan_set_option: value out of range");
      p->tune.potrf_slots = (int)value;
      return 0;
    case DGP_OPT_REFINE:
      if (p->dtype != DGP_F32 && value) return fail(DGP_E_ARG, "dgp_plan_set_option: refinement applies to float32 plans");
      p->refine = value ? 1 : 0;
      return 0;
    default:
      return fail(DGP_E_ARG, "dgp_plan_set_option: unknown option");
  }
}
int dgp_plan_get_option(const dgp_plan* p, int key, int64_t* value) {
  if (!p || !value) return fail(DGP_E_ARG, "dgp_plan_get_option: null argument");
  switch (key) {
    case DGP_OPT_LAUUM64_MAX_TILES: *value = p->tune.lauum64_max_tiles; return 0;
    case DGP_OPT_SYRK_SLOTS: *value = p->tune.syrk_slots; return 0;
    case DGP_OPT_TRTRI_SMALL: *value = p->tune.trtri_small; return 0;
    case DGP_OPT_REFINE: *value = p->refine; return 0;
    case DGP_OPT_SYRK_ORDER: *value = p->tune.syrk_super; return 0;
    case DGP_OPT_LAUUM_ORDER: *value = p->tune.lauum_super; return 0;
    case DGP_OPT_CHAIN_YIELD: *value = p->tune.chain_yield; return 0;
    case DGP_OPT_FUSED_GRAD: *value = p->tune.fused_grad; return 0;
    case DGP_OPT_GROUP_GEMM: *value = p->tune.group_gemm; return 0;
    case DGP_OPT_POTRF_SCHEDULE:  // (the selector's choice for this plan's shape unless set)
      *value = p->tune.potrf_schedule < 0 ? (p->B >= 4 ? potrf_schedule_auto(p->B, p->N / DGP_TILE_HOST, p->elem) : 0) : p->tune.potrf_schedule;
      return 0;
    case DGP_OPT_POTRF_SWEEP: *value = p->tune.potrf_sweep; return 0;
    case DGP_OPT_POTRF_SOLVE: *value = p->tune.potrf_solve; return 0;
    case DGP_OPT_POTRF_OVERLAP: *value = p->tune.potrf_overlap; return 0;
    case DGP_OPT_POTRF_SLOTS: *value = p->tune.potrf_slots; return 0;
    case DGP_OPT_POTRF_TAIL: *value = p->tune.potrf_tail; return 0;
    case DGP_OPT_POTRF_TAIL_SWEEP: *value = p->tune.potrf_tail_sweep; return 0;
    default: return fail(DGP_E_ARG, "dgp_plan_get_option: unknown option");
  }
}

int dgp_plan_set_lookahead(dgp_plan* p, int level) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  p->lookahead = level ? default_lookahead() : 0;
  p->early = level >= 2 && !getenv("DGP_NO_EARLY_TRTRI");
  return 0;
}

size_t dgp_plan_site_stride_bytes(const dgp_plan* p) { return p ? layout(p).total : 0; }

int dgp_plan_buffer(const dgp_plan* p, int which, void** dev_ptr, int64_t* ld) {
  if (!p || !dev_ptr || !p->ws) return fail(DGP_E_ARG, "dgp_plan_buffer: null / no workspace");
  void* q = nullptr;
  switch (which) {
    case DGP_BUF_XT: q = p->Xt; break;
    case DGP_BUF_A: q = p->A; break;
    case DGP_BUF_T: q = p->Tm; break;
    case DGP_BUF_S: q = p->S; break;
    case DGP_BUF_Z: q = p->z; break;
    case DGP_BUF_ALPHA: q = p->alpha; break;
    case DGP_BUF_INFO: q = p->info; break;
    case DGP_BUF_SCAL: q = p->scal; break;
    default: return fail(DGP_E_ARG, "dgp_plan_buffer: unknown buffer");
  }
  *dev_ptr = q;
  if (ld) *ld = p->N;
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// The library's internal streams belong to the CALLER'S stream, not to a plan: every plan driven from one stream (the
// usual case: torch's current stream) uses the same three -- bulk updates (lowest priority), rest of the split panel
// chain (highest), early inverse (lowest).  A process has few hardware queues (4 by default); streams beyond that share
// one, and kernels of streams that share a queue run one after the other.  With a stream set per PLAN, a process that had
// created a second plan found the rest stream of the split chain behind the bulk stream in one queue: the critical
// kernels then wait for whole bulk launches (measured: a single n = 8192 fit went from 12.3 to 20 ms as soon as a batched
// plan existed in the process).  Plans driven from DIFFERENT streams (sites.py::fit_sites) still get a set each.  The
// streams live as long as the process.
struct StreamSet {
  hipStream_t bulk = nullptr, rest = nullptr, early = nullptr;
};
static StreamSet* stream_set(hipStream_t caller) {
  static std::mutex mtx;
  static std::vector<std::pair<std::pair<int, hipStream_t>, StreamSet*>> sets;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(mtx);
  for (auto& e : sets)
    if (e.first.first == dev && e.first.second == caller) return e.second;
  StreamSet* st = new (std::nothrow) StreamSet();
  if (!st) return nullptr;
  sets.push_back({{dev, caller}, st});
  return st;
}
static int make_stream(hipStream_t* out, bool high) {
  if (*out) return 0;
  int least = 0, greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
  hipError_t e = hipStreamCreateWithPriority(out, hipStreamNonBlocking, high ? greatest : least);
  return e == hipSuccess ? 0 : hipfail(e, "hipStreamCreateWithPriority");
}

// ---- shader-clock probe ---------------------------------------------------------------------------------------------
// MI355X lowers its clock under an MFMA-dense load (MI355X_MICROARCH.md "DVFS give-back"), so a kernel's fraction of the
// 2.4 GHz peak mixes two things: how full it keeps the MFMA pipe and which clock the chip held.  This probe separates
// them WITHOUT touching a product kernel: a few one-wave workgroups stay resident for `ticks` of the 100 MHz wall clock
// and stamp the shader-cycle counter (s_memtime) and the wall clock (s_memrealtime) at both ends; the caller runs the
// load (e.g. back-to-back lauum launches) on another stream meanwhile.  clock = d s_memtime / d s_memrealtime x 100 MHz
// per workgroup (consecutive workgroup ids land on consecutive XCDs: 8 or more cover every XCD).  The stamps go to a
// buffer of their own; no product value is computed from them.
__global__ __launch_bounds__(64) void clock_probe_kernel(unsigned long long* __restrict__ out, long long ticks) {
  const long long r0 = wall_clock64();
  const long long s0 = clock64();
  while (wall_clock64() - r0 < ticks) __builtin_amdgcn_s_sleep(64);
  const long long s1 = clock64();
  const long long r1 = wall_clock64();
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = (unsigned long long)(s1 - s0);
    out[2 * blockIdx.x + 1] = (unsigned long long)(r1 - r0);
  }
}


static int ensure_async(dgp_plan* p, hipStream_t s) {
  if (!p->lookahead) return 0;
  // the bulk trailing updates run at the LOWEST priority so that the latency-critical panel chain on
  // the caller's stream gets the CUs first whenever both have workgroups ready
  StreamSet* st = stream_set(s);
  if (!st) return fail(DGP_E_ARG, "out of host memory");
  int rc = make_stream(&st->bulk, false);
  if (rc) return rc;
  p->s2 = st->bulk;
  if (p->ev) return 0;
  hipError_t e;
  p->nev = 3 * (int)(p->N / DGP_TILE_HOST);  // group-ahead schedule: P, U; split chain: ED, ER, U
  p->ev = new (std::nothrow) hipEvent_t[p->nev];
  if (!p->ev) return fail(DGP_E_ARG, "out of host memory");
  for (int i = 0; i < p->nev; ++i) {
    e = hipEventCreateWithFlags(&p->ev[i], hipEventDisableTiming);
    if (e != hipSuccess) return hipfail(e, "hipEventCreateWithFlags");
  }
  return 0;
}

// The split panel chain (critical tile on the caller's stream, rest of the chain on `sc`): one site.  Large matrices start in the
// group schedule (groups of 2 / 4 / 8 panels, group_size()) and hand over for their chain-bound tail (split_start()).
// DGP_SPLIT_CHAIN=0 selects the single-stream chain (A/B measurements, the bitwise-equality tests); read at every call.
static bool split_applies(const dgp_plan* p) {
  const char* e = getenv("DGP_SPLIT_CHAIN");
  if (e && atoi(e) == 0) return false;
  const long nbk = p->N / DGP_TILE_HOST;
  return p->B == 1 && p->lookahead && nbk >= 4 && group_size(p->lookahead, p->B, nbk) % 2 == 0;  // (DGP_GROUP may ask for odd groups)
}
// first block column of the split chain: the earliest even k from which a bulk launch (all tiles right of the pair) is at
// most DGP_SPLIT_TILES tiles (default 768 = 1.5 rounds of the 512 workgroup slots): before that the factorisation is bound
// by its bulk launches and every chain kernel queues behind them whatever the schedule
static int split_start(const dgp_plan* p) {
  const char* e = getenv("DGP_SPLIT_TILES");
  const long cap = e ? atol(e) : 768;
  const int nbk = (int)(p->N / DGP_TILE_HOST);
  int k = 0;
  while (k + 4 <= nbk && (long)(nbk - k - 3) * (nbk - k - 2) / 2 > cap) k += 2;
  return k;
}
static int ensure_split(dgp_plan* p, hipStream_t s) {
  if (!split_applies(p)) return 0;
  StreamSet* st = stream_set(s);
  if (!st) return fail(DGP_E_ARG, "out of host memory");
  const int rc = make_stream(&st->rest, true);
  if (rc) return rc;
  p->sc = st->rest;
  return 0;
}

// the third stream exists only for plans that use it: every extra stream per plan costs throughput once
// several plans share the GPU (measured 86 -> 78 fits/s with two plans), so batched callers select level 1
static bool early_applies(const dgp_plan* p) {
  if (p->B != 1) return false;  // a batched plan's sites already fill each other's idle CUs
  // measured (fp64, one site): n = 2048 -1 %, 4096 -3 %, 8192 -6 %, 12288 +0.3 %, 16384 +0.8 %, 32768 (fp32) +6 %:
  // beyond ~10k the factorisation is bound by its bulk updates, not by the panel chain, and has no idle tail
  const int nbk = (int)(p->N / DGP_TILE_HOST);
  return p->early && p->lookahead >= 2 && nbk >= 16 && nbk <= 80;
}
static int ensure_early(dgp_plan* p, hipStream_t s) {
  if (!early_applies(p)) return 0;  // an idle extra stream is not free either (n = 32768: 293 -> 305 ms)
  StreamSet* st = stream_set(s);
  if (!st) return fail(DGP_E_ARG, "out of host memory");
  const int rc = make_stream(&st->early, false);
  if (rc) return rc;
  p->s3 = st->early;
  if (p->have_xev) return 0;
  hipError_t e;
  for (int i = 0; i < 8; ++i) {
    e = hipEventCreateWithFlags(&p->xev[i], hipEventDisableTiming);
    if (e != hipSuccess) return hipfail(e, "hipEventCreateWithFlags");
  }
  p->have_xev = 1;
  return 0;
}

static int ensure_timing(dgp_plan* p) {
  if (!p->timing || p->tev) return 0;
  p->tev = new (std::nothrow) hipEvent_t[2 * TS_COUNT];
  p->nsev = 2 * (int)(p->N / DGP_TILE_HOST);
  p->sev = new (std::nothrow) hipEvent_t[p->nsev];
  if (!p->tev || !p->sev) return fail(DGP_E_ARG, "out of host memory");
  for (int i = 0; i < 2 * TS_COUNT; ++i) {
    hipError_t e = hipEventCreate(&p->tev[i]);
    if (e != hipSuccess) return hipfail(e, "hipEventCreate");
  }
  for (int i = 0; i < p->nsev; ++i) {
    hipError_t e = hipEventCreate(&p->sev[i]);
    if (e != hipSuccess) return hipfail(e, "hipEventCreate");
  }
  return 0;
}
static void tick(dgp_plan* p, int stage, int stop, hipStream_t s) {
  if (p->timing && p->tev) (void)hipEventRecord(p->tev[2 * stage + stop], s);
}

// The tail of a fit step in ONE launch: dnoise_i = 1/2 (S_ii - alpha_i^2), dr = alpha, and the result row -- NLL,
// log-determinant, quadratic form, pivot status, and the reductions of dNLL/dr (= alpha) and dNLL/dnoise that a host-side
// mean / noise model needs for its gradients (sum dr, sum dr w0, sum dr w1, sum dnoise), so that the host never reduces
// device vectors.  Every workgroup handles 256 observations and leaves its partial sums in `part`; the last one to
// finish (ticket counter info[1], reset for the next step) adds them up in workgroup order and writes the row: the
// result does not depend on scheduling.  zero_grad (dgp_factorize): one workgroup, scalars only.
template <typename T>
__global__ __launch_bounds__(256) void finish_kernel(const T* scal, int* info, long n, int ntheta, int zero_grad, T* out,
                                                     long bs, long ibs, const int* ns, const T* alpha, const T* w, const T* S,
                                                     long N, T* dnoise, T* dr, T* part) {
  const long nfull = n;
  n = site_n(ns, (int)n);
  scal = site(scal, bs);
  info = site(info, ibs);
  alpha = site(alpha, bs);
  S = site(S, bs);
  part = site(part, bs);
  if (dnoise) dnoise = site(dnoise, nfull);
  if (dr) dr = site(dr, nfull);
  if (w) w = site(w, 2 * nfull);  // [site][2][n]
  out = site(out, (long)DGP_OUT_LEN);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  __shared__ T red[4][4];
  __shared__ int last;
  T v[4] = {T(0), T(0), T(0), T(0)};
  if (!zero_grad) {
    const long i = (long)blockIdx.x * 256 + t;
    if (i < nfull) {
      const T a = alpha[i];
      const T dn = i < n ? T(0.5) * (S[i * N + i] - a * a) : T(0);
      if (dnoise) dnoise[i] = dn;
      if (dr) dr[i] = a;
      if (i < n) {
        v[0] = a;
        if (w) {
          v[1] = a * w[i];
          v[2] = a * w[nfull + i];
        }
        v[3] = dn;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const T sum = wave_sum(v[q]);
      if (lane == 0) red[wv][q] = sum;
    }
    __syncthreads();
    if (t < 4) part[(long)blockIdx.x * 4 + t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
    __threadfence();
  }
  if (t == 0) last = (gridDim.x == 1) || (atomicAdd(&info[1], 1) == (int)gridDim.x - 1);
  __syncthreads();
  if (!last) return;
  __threadfence();
  if (t == 0) info[1] = 0;
  if (t < 4) {
    T total = T(0);
    if (!zero_grad)
      for (unsigned g = 0; g < gridDim.x; ++g) total += ((const volatile T*)part)[(long)g * 4 + t];  // other workgroups' stores
    red[0][t] = total;
  }
  __syncthreads();
  if (t == 0) {
    // fp32 plans: the log-determinant (summed over the diagonal blocks in double, dgp_diag.h) and the quadratic form were accumulated in
    // double and sit unrounded in the scalar block's double slots (elements 2..3 and 4..5); the three terms of the NLL
    // -- which cancel to a small number when the noise is small -- are added in double and rounded once
    double logdet = (double)scal[0], quad = (double)scal[1];
    if (sizeof(T) == 4) {
      logdet = *reinterpret_cast<const double*>(scal + 2);
      quad = *reinterpret_cast<const double*>(scal + 4);
    }
    if (info[0] < 0) quad = __builtin_nan("");  // the split chain gave up waiting (dgp_chol.hip::chain_wait): no factor
    out[DGP_OUT_NLL] = (T)(0.5 * quad + 0.5 * logdet + 0.5 * 1.83787706640934548356 * (double)n);
    out[DGP_OUT_QUAD] = (T)quad;
    out[DGP_OUT_LOGDET] = (T)logdet;
    out[DGP_OUT_INFO] = (T)info[0];
  }
  if (zero_grad && t >= DGP_OUT_DTHETA && t < DGP_OUT_LEN) out[t] = T(0);
  if (!zero_grad && t >= DGP_OUT_DTHETA + ntheta && t < DGP_OUT_LEN) out[t] = t >= DGP_OUT_SUM_DR ? red[0][t - DGP_OUT_SUM_DR] : T(0);
}


template <typename T>
static Batch batch_of(const dgp_plan* p) {
  Batch bt;
  bt.B = p->B;
  bt.ws = (long)(p->site_bytes / sizeof(T));  // layout offsets are multiples of 256 bytes
  bt.ns = p->nsite;
  bt.tune = &p->tune;
  bt.W = p->S;  // scratch of the factorisation's group inverse (S is free until trtri / lauum use it)
  return bt;
}
template <typename T>
static int run_gram(dgp_plan* p, const double* theta, const void* noise, hipStream_t s) {
  p->pre_ready = 1;
  void* staging = p->pre ? p->ring.acquire(pre_scratch_bytes(p->B)) : nullptr;
  const int rc = gram_sym<T>(p->model, p->d, (const T*)p->Xt, p->N, (int)p->n, theta, (const T*)noise, (T*)p->A, s,
                             batch_of<T>(p), p->pre, staging);
  if (staging) p->ring.commit(s);
  return rc;
}
// The factorisation, by the split chain or the group schedule.  nck > 0: after block column ck[c] is final the schedule
// records ck_ev[c] and calls on_ck(ctx, c) from its enqueue loop (fit_step's early inverse).
template <typename T>
static int run_potrf(dgp_plan* p, hipStream_t s, int nck = 0, const int* ck = nullptr, hipEvent_t* ck_ev = nullptr,
                     void (*on_ck)(void*, int) = nullptr, void* ctx = nullptr) {
  int rc = ensure_async(p, s);
  if (rc) return rc;
  if ((rc = ensure_timing(p)) || (rc = ensure_split(p, s))) return rc;
  const int group = group_size(p->lookahead, p->B, p->N / DGP_TILE_HOST);
  PotrfObservers obs;
  obs.syrk_ev = p->timing ? p->sev : nullptr;
  obs.syrk_pool = p->nsev / 2;
  obs.nck = nck;
  obs.ck_blocks = ck;
  obs.ck_ev = ck_ev;
  obs.on_ck = on_ck;
  obs.ck_ctx = ctx;
  if (split_applies(p) && p->sc)
    rc = potrf_split<T>((T*)p->A, p->N, (T*)p->Tm, (T*)p->scal, p->info, (T*)p->snap, s, p->sc, p->s2, p->ev, &obs, split_start(p), group,
                        &p->tune);
  else
    rc = potrf<T>((T*)p->A, p->N, (T*)p->Tm, (T*)p->scal, p->info, group, s, p->s2, p->ev, &obs, batch_of<T>(p));
  p->n_syrk = obs.n_syrk;
  p->syrk_flop = obs.syrk_flop;
  return rc;
}
template <typename T>
static int run_trtri(dgp_plan* p, hipStream_t s) {
  return trtri<T>((const T*)p->A, nullptr, p->N, (T*)p->Tm, (T*)p->S /* scratch W aliases S */, s, batch_of<T>(p));
}
template <typename T>
static int run_lauum(dgp_plan* p, hipStream_t s) {
  return lauum<T>((const T*)p->Tm, p->N, (T*)p->S, s, batch_of<T>(p));
}
template <typename T>
static int run_solve(dgp_plan* p, const void* r, hipStream_t s) {
  return solve<T>((const T*)p->Tm, p->N, (const T*)r, (int)p->n, (T*)p->z, (T*)p->alpha, (T*)p->spart,
                  (T*)p->scal + 1, s, batch_of<T>(p));
}
// fp32 plans: one step of iterative refinement of alpha and of the quadratic form with an fp64 residual (SURVEY.md section
// 8d's fp32 row as written; the reference trains in float32, src/discontinuum/engines/gpytorch.py:221-222, 350-353).
// The factor is stored in fp32, so alpha0 = T^T T r carries cond(K^) eps32 (2.4e-3 at config 3) and the quadratic form
// 1e-5 of itself -- more than the whole NLL tolerance when its three terms cancel.  rho = r - K^ alpha0 in double with K^
// re-evaluated on the fly (gram_residual), delta from the fp32 factor, alpha = alpha0 + delta, quad second-order accurate
// (refine_finish_kernel).  The scratch lives in S, which is free between the solves and lauum (trtri's W is consumed).
template <typename T>
static int run_refine(dgp_plan* p, const double* theta, const void* r, const void* noise, hipStream_t s) {
  if constexpr (sizeof(T) != 4) {
    return 0;
  } else {
    if (!p->refine) return 0;
    const long N = p->N;
    const size_t nb = (size_t)(N / 64), part_bytes = nb * nb * 64 * sizeof(double);
    if (gram_residual_scratch_bytes(N) > (size_t)N * N * sizeof(float)) return 0;  // (never: N >= 128)
    char* base = (char*)p->S;
    double* part = (double*)base;
    double* rho64 = (double*)(base + part_bytes);
    float* rho32 = (float*)(base + part_bytes + (size_t)N * sizeof(double));
    float* delta = rho32 + N;
    const Batch bt = batch_of<float>(p);
    const long ps = bt.ws / 2;  // site stride of S in doubles (bt.ws floats, a multiple of 64)
    void* staging = p->pre2 ? p->ring.acquire(pre_scratch_bytes(p->B)) : nullptr;
    int rc = gram_residual<float>(p->model, p->d, (const float*)p->Xt, N, (int)p->n, theta, (const float*)noise, (const float*)r,
                                  (const float*)p->alpha, part, rho64, rho32, s, bt, ps, bt.ws, p->pre2, staging);
    if (staging) p->ring.commit(s);
    if (rc) return rc;
    return refine_solve<float>((const float*)p->Tm, N, (const float*)r, (int)p->n, rho64, rho32, (float*)p->z, delta,
                               (float*)p->alpha, (float*)p->spart, (float*)p->scal + 1, s, bt, ps, bt.ws);
  }
}

template <typename T>
static int run_grad(dgp_plan* p, const double* theta, void* dtheta, hipStream_t s) {
  return gram_grad<T>(p->model, p->d, (const T*)p->Xt, p->N, (int)p->n, theta, (const T*)p->S, (const T*)p->alpha,
                      (T*)p->gpart, (T*)dtheta, s, batch_of<T>(p), DGP_OUT_LEN, p->pre, p->pre_ready != 0);
}

// Whether the two solves run BESIDE lauum on the bulk stream (lowest priority: the solve's workgroups fill whatever slots lauum's grid
// leaves) instead of in front of it on the caller's stream.  Needs the plan's event pool (lookahead >= 1).  Measured on one box in
// alternating processes (scripts/env_ab.py, wall ms per step, in front / bulk stream / a highest-priority stream of their own):
// 32 x n = 8192 274.3 / 273.8 / 274.4 (lauum itself 81.0 -> 83.3 with the solves beside it: its three workgroups per CU leave a trmv
// wave no registers, so the solves take slots, not idle resources), 64 x n = 4096 80.56 / 79.30 / 79.59 (-1.6 %), one site n = 8192
// 11.85 / 11.84 / 11.81; bitwise the same results.  Hence only for 1024 <= N <= 6144: at the headline size the step gains 0.2 %
// (below the 1 % bar) while lauum -- the kernel the roofline is quoted on -- reads 3-4 % slower for sharing the GPU (84.8 against
// 82.4 ms alone, profiles/r05_lauum_three_ways.txt); and not below N = 1024: at the reference's own site size, n = 300, the step is
// ~0.3 ms of launches and the two cross-stream dependencies cost more than the overlap gains: 0.306 -> 0.334 ms; n = 1024
// 0.705 -> 0.681, 2048 1.319 -> 1.270, 128 x n = 2048 26.24 -> 25.62.  (Figures of the two-pass trmv kernels.  With the one-pass
// row kernel, dgp_chol.hip::trsv_rows_kernel, the window stands: 64 x n = 4096 steps 77.78 -> 76.67 ms with it on the bulk stream.)
template <typename T>
static bool solve_overlap(const dgp_plan* p) {
  if (p->N < 1024 || p->N > 6144 || !p->lookahead || !p->ev || p->nev < 2 || !p->s2) return false;
  return !(sizeof(T) == 4 && p->refine);
}

template <typename T>
static int fit_step(dgp_plan* p, const double* theta, const void* r, const void* noise, void* out, void* dr,
                    void* dnoise, int with_grad, hipStream_t s) {
  int rc;
  if ((rc = ensure_timing(p))) return rc;
  tick(p, TS_GRAM, 0, s);
  if ((rc = run_gram<T>(p, theta, noise, s))) return rc;
  tick(p, TS_GRAM, 1, s);
  if ((rc = ensure_async(p, s)) || (rc = ensure_early(p, s))) return rc;
  tick(p, TS_POTRF, 0, s);
  const int nbk = (int)(p->N / DGP_TILE_HOST);
  const bool early = early_applies(p) && p->s3 != nullptr;
  const Batch bt = batch_of<T>(p);
  if (early) {
    // The factorisation's tail is a sequential panel chain that leaves most CUs idle, and the inverse's level
    // recursion only needs the block columns that are already final: issue it piecewise on s3 behind
    // checkpoints at 1/2, 3/4 and 7/8 of the columns (W-steps as soon as the left half of a group is final).
    struct Early {
      dgp_plan* p;
      int ck[3];
      TrtriProgress st;
      int rc;
    } ctx{p, {nbk / 2, 3 * nbk / 4, 7 * nbk / 8}, {}, 0};
    auto on_ck = [](void* v, int c) {  // runs inside the factorisation's enqueue loop, right after checkpoint c
      Early* e = (Early*)v;
      hipStreamWaitEvent(e->p->s3, e->p->xev[c], 0);
      const int rc = trtri_advance<T>((const T*)e->p->A, e->p->N, (T*)e->p->Tm, (T*)e->p->S, e->ck[c], &e->st,
                                      e->p->s3, EARLY_WG_CAP, e->p->info + EARLY_CTR0, EARLY_CTR_PAIRS,
                                      EARLY_RESERVED_CUS, batch_of<T>(e->p));
      if (rc && !e->rc) e->rc = rc;
    };
    if ((rc = run_potrf<T>(p, s, 3, ctx.ck, p->xev, on_ck, &ctx)) || (rc = ctx.rc)) return rc;
    tick(p, TS_POTRF, 1, s);
    tick(p, TS_TRTRI, 0, s);
    hipEventRecord(p->xev[3], s);  // factorisation complete (s has joined the bulk stream)
    hipStreamWaitEvent(p->s3, p->xev[3], 0);
    if ((rc = trtri_advance<T>((const T*)p->A, p->N, (T*)p->Tm, (T*)p->S, nbk, &ctx.st, p->s3, 0, nullptr, 0, 0, bt)))
      return rc;
    hipEventRecord(p->xev[4], p->s3);
    hipStreamWaitEvent(s, p->xev[4], 0);
    tick(p, TS_TRTRI, 1, s);
  } else {
    if ((rc = run_potrf<T>(p, s))) return rc;
    tick(p, TS_POTRF, 1, s);
    tick(p, TS_TRTRI, 0, s);
    if ((rc = run_trtri<T>(p, s))) return rc;
    tick(p, TS_TRTRI, 1, s);
  }
  // The two triangular solves (HBM-bound: z = T r and alpha = T^T z from one read of T) need T and r only, and K^^-1 = T^T T
  // (MFMA-bound) needs T only: with a second stream at hand the solves run BESIDE lauum instead of in front of it and join
  // before the gradient contraction, which needs both.  fp32 plans with the refinement keep the order: its scratch is S.
  // (the FUSED kernel -- K^^-1 with the gradient contraction in its epilogue, dgp_fused.hip -- needs alpha before it
  // starts: the solves then stay in front of it on the caller's stream)
  const bool fused = with_grad && p->tune.fused_grad && lauum_grad_applies(p->model, p->N, bt);
  const bool ov = with_grad && !fused && solve_overlap<T>(p);
  hipStream_t ss = ov ? p->s2 : s;
  if (ov) {
    hipEventRecord(p->ev[0], s);
    hipStreamWaitEvent(ss, p->ev[0], 0);
  }
  tick(p, TS_SOLVE, 0, ss);
  if ((rc = run_solve<T>(p, r, ss))) return rc;
  if ((rc = run_refine<T>(p, theta, r, noise, ss))) return rc;
  tick(p, TS_SOLVE, 1, ss);
  if (ov) hipEventRecord(p->ev[1], ss);
  p->timed_valid = 0;
  p->have_inverse = 0;
  if (!with_grad && ov) hipStreamWaitEvent(s, p->ev[1], 0);
  if (fused) {
    // TIME_LAUUM then covers the fused launch (N^3/3 flop on MFMA + the contraction's vector work beside it), TIME_GRAD the
    // second reduction stage alone
    tick(p, TS_LAUUM, 0, s);
    void* staging = (p->pre && !p->pre_ready) ? p->ring.acquire(pre_scratch_bytes(p->B)) : nullptr;
    rc = lauum_grad<T>(p->model, p->d, (const T*)p->Tm, p->N, (T*)p->S, (const T*)p->Xt, (int)p->n, theta, (const T*)p->alpha,
                       (T*)p->gpart, (T*)out + DGP_OUT_DTHETA, s, bt, DGP_OUT_LEN, p->pre, p->pre_ready != 0, staging);
    if (staging) p->ring.commit(s);
    if (rc) return rc;
    p->pre_ready = 1;
    tick(p, TS_LAUUM, 1, s);
    tick(p, TS_GRAD, 0, s);
    tick(p, TS_GRAD, 1, s);
    p->timed_valid = p->timing && p->tev;
    p->have_inverse = 1;
  } else if (with_grad) {
    tick(p, TS_LAUUM, 0, s);
    if ((rc = run_lauum<T>(p, s))) return rc;
    tick(p, TS_LAUUM, 1, s);
    if (ov) hipStreamWaitEvent(s, p->ev[1], 0);
    tick(p, TS_GRAD, 0, s);
    if ((rc = run_grad<T>(p, theta, (T*)out + DGP_OUT_DTHETA, s))) return rc;
    tick(p, TS_GRAD, 1, s);
    p->timed_valid = p->timing && p->tev;
    p->have_inverse = 1;
  }
  const unsigned nwg = with_grad ? (unsigned)((p->n + 255) / 256) : 1u;
  finish_kernel<T><<<dim3(nwg, 1, (unsigned)bt.B), 256, 0, s>>>(
      (const T*)p->scal, p->info, (long)p->n, p->ntheta, !with_grad, (T*)out, bt.ws, bt.ws * (long)sizeof(T) / (long)sizeof(int), bt.ns,
      (const T*)p->alpha, (const T*)(with_grad ? p->dr_w : nullptr), (const T*)p->S, p->N, (T*)(with_grad ? dnoise : nullptr),
      (T*)(with_grad ? dr : nullptr), (T*)p->spart);
  p->have_factor = 1;
  return (int)hipGetLastError();
}

// ---- inference on the factorisation a plan holds.  Batched plans run every launch once for all sites (gridDim.z =
// sites, like the fit step): the caller's work area holds one slice per site (site stride = the single-site size).
static size_t predict_site_bytes(const dgp_plan* p, int64_t m) {
  const size_t M = (size_t)round_up(m, DGP_TILE_HOST), e = p->elem;
  return align_up(e * M * p->d) + 2 * align_up(e * (size_t)p->N * M) + 3 * align_up(e * M) + align_up(e * 2 * PREDICT_SPLIT * M);
}
// hyperparameters of a batch of more than 8 sites travel through the plan's device scratch + a pinned staging slot
struct PreSlot {
  dgp_plan* p;
  void* staging;
  hipStream_t s;
  PreSlot(dgp_plan* plan, hipStream_t st) : p(plan), staging(plan->pre ? plan->ring.acquire(pre_scratch_bytes(plan->B)) : nullptr), s(st) {
    plan->pre_ready = 0;  // the fit step's copy of the hyperparameters is overwritten
  }
  ~PreSlot() {
    if (staging) p->ring.commit(s);
  }
};

template <typename T>
static int cross(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* Ks, hipStream_t s, long wbs = 0) {
  const long M = round_up(m, DGP_TILE_HOST);
  Batch wb;  // the test points: [B][m][d] -> SoA in the work area
  wb.B = p->B;
  wb.ws = wbs;
  int rc = pack_x<T>((const T*)Xs, (int)m, p->d, M, (T*)work, s, wb);
  if (rc) return rc;
  PreSlot slot(p, s);
  return gram_cross<T>(p->model, p->d, (const T*)p->Xt, p->N, (int)p->n, (const T*)work, M, (int)m, theta, (T*)Ks, s, batch_of<T>(p), wbs,
                       p->pre, slot.staging);
}

template <typename T>
__global__ void copy_rows_kernel(const T* src, long n, T* dst, long src_stride) {  // dst [site][n] <- src at src_stride
  src = site(src, src_stride);
  dst = site(dst, n);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

template <typename T>
static int predict_common(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* mean, T** V_out, T** Xst_out,
                          T** vpad_out, long* wbs_out, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST);
  const size_t e = sizeof(T);
  const long wbs = p->B > 1 ? (long)(predict_site_bytes(p, m) / e) : 0;
  char* w = (char*)work;
  T* Xst = (T*)w; w += align_up(e * M * p->d);
  T* Ks = (T*)w; w += align_up(e * (size_t)p->N * M);
  T* V = (T*)w; w += align_up(e * (size_t)p->N * M);
  T* kss = (T*)w; w += align_up(e * M);
  T* mpad = (T*)w; w += align_up(e * M);
  T* vpad = (T*)w; w += align_up(e * M);
  T* part = (T*)w;
  const unsigned Bz = (unsigned)p->B;
  int rc = cross<T>(p, theta, Xs, m, Xst, Ks, s, wbs);
  if (rc) return rc;
  Batch wb;
  wb.B = p->B;
  if ((rc = gram_diag<T>(p->model, p->d, Xst, M, (int)m, theta, kss, s, wb, wbs, p->pre))) return rc;
  if ((rc = predict_var<T>((const T*)p->Tm, p->N, Ks, M, V, (const T*)p->alpha, kss, part, mpad, vpad, s, batch_of<T>(p), wbs))) return rc;
  copy_rows_kernel<T><<<dim3((unsigned)((m + 255) / 256), 1, Bz), 256, 0, s>>>(mpad, m, (T*)mean, wbs);
  *V_out = V;
  *Xst_out = Xst;
  *vpad_out = vpad;
  *wbs_out = wbs;
  return (int)hipGetLastError();
}

template <typename T>
static int predict(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* mean, void* var,
                   hipStream_t s) {
  T *V, *Xst, *vpad;
  long wbs;
  int rc = predict_common<T>(p, theta, Xs, m, work, mean, &V, &Xst, &vpad, &wbs, s);
  if (rc) return rc;
  copy_rows_kernel<T><<<dim3((unsigned)((m + 255) / 256), 1, (unsigned)p->B), 256, 0, s>>>(vpad, m, (T*)var, wbs);
  return (int)hipGetLastError();
}

template <typename T>
static int post_cov(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* mean, void* cov,
                    hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST);
  T *V, *Xst, *vpad;
  long wbs;
  int rc = predict_common<T>(p, theta, Xs, m, work, mean, &V, &Xst, &vpad, &wbs, s);
  if (rc) return rc;
  // zero "noise" for K(Xs, Xs); a batched plan's sites keep theirs at the work area's site stride
  hipError_t he = hipMemset2DAsync(vpad, sizeof(T) * (size_t)(wbs > 0 ? wbs : M), 0, sizeof(T) * M, (size_t)p->B, s);
  if (he != hipSuccess) return (int)he;
  Batch wb;
  wb.B = p->B;
  wb.ws = wbs;
  if ((rc = gram_sym<T>(p->model, p->d, Xst, M, (int)m, theta, vpad, (T*)cov, s, wb, p->pre, nullptr, M * M, wbs, true))) return rc;
  return posterior_cov<T>(V, p->N, M, (T*)cov, s, p->B, wbs);
}

struct VjpLayout {
  size_t Xst, Ks, g, beta, part, spart, total;
};
static VjpLayout vjp_layout(const dgp_plan* p, int64_t m) {
  const size_t M = (size_t)round_up(m, DGP_TILE_HOST), e = p->elem, N = (size_t)p->N;
  const size_t nb = N / 64, blocks_sym = nb * (nb + 1) / 2, blocks_cross = (M / 64) * nb;
  VjpLayout L;
  size_t o = 0;
  L.Xst = o; o += align_up(e * M * p->d);
  L.Ks = o; o += align_up(e * N * M);
  L.g = o; o += align_up(e * (N > M ? N : M));
  L.beta = o; o += align_up(e * N);
  L.part = o; o += align_up(e * 24 * (blocks_sym > blocks_cross ? blocks_sym : blocks_cross));
  L.spart = o; o += align_up(e * (size_t)solve_partials(p->N));
  L.total = o;
  return L;
}

template <typename T>
__global__ void matvec_cols_kernel(const T* Ks, long N, long Mp, int n, const T* alpha, T* out, long bs, long wbs, const int* ns) {
  // out[j] = sum_i Ks[i][j] alpha_i : one thread per column, coalesced across columns
  Ks = site(Ks, wbs);
  out = site(out, wbs);
  alpha = site(alpha, bs);
  n = site_n(ns, n);
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= Mp) return;
  T acc = T(0);
  for (long i = 0; i < n; ++i) acc += Ks[i * Mp + j] * alpha[i];
  out[j] = acc;
}

template <typename T>
static int predict_mean(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* mean,
                        hipStream_t s) {
  const VjpLayout L = vjp_layout(p, m);
  const long M = round_up(m, DGP_TILE_HOST);
  const long wbs = p->B > 1 ? (long)(L.total / sizeof(T)) : 0;
  const Batch bt = batch_of<T>(p);
  char* w = (char*)work;
  int rc = cross<T>(p, theta, Xs, m, w + L.Xst, w + L.Ks, s, wbs);
  if (rc) return rc;
  matvec_cols_kernel<T><<<dim3((unsigned)((M + 255) / 256), 1, (unsigned)p->B), 256, 0, s>>>((const T*)(w + L.Ks), p->N, M, (int)p->n,
                                                                                           (const T*)p->alpha, (T*)(w + L.g), bt.ws, wbs, bt.ns);
  copy_rows_kernel<T><<<dim3((unsigned)((m + 255) / 256), 1, (unsigned)p->B), 256, 0, s>>>((const T*)(w + L.g), m, (T*)mean, wbs);
  return (int)hipGetLastError();
}

template <typename T>
static int mean_vjp(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* wts, void* work,
                    void* dtheta, void* dr, void* dnoise, hipStream_t s) {
  const VjpLayout L = vjp_layout(p, m);
  const long M = round_up(m, DGP_TILE_HOST);
  const long wbs = p->B > 1 ? (long)(L.total / sizeof(T)) : 0;
  const Batch bt = batch_of<T>(p);
  char* w = (char*)work;
  T* Xst = (T*)(w + L.Xst);
  T* Ks = (T*)(w + L.Ks);
  T* g = (T*)(w + L.g);
  T* beta = (T*)(w + L.beta);
  int rc = cross<T>(p, theta, Xs, m, Xst, Ks, s, wbs);
  if (rc) return rc;
  if ((rc = gemv_rows<T>(Ks, p->N, M, (int)m, (const T*)wts, g, s, p->B, wbs))) return rc;   // g = K(X, X*) w
  if ((rc = symv_lower<T>((const T*)p->S, p->N, g, (int)p->n, (const T*)p->alpha, beta, (T*)(w + L.spart),
                          (T*)dnoise, s, bt, wbs)))                                         // beta = K^^-1 g
    return rc;
  if (dr) copy_rows_kernel<T><<<dim3((unsigned)((p->n + 255) / 256), 1, (unsigned)p->B), 256, 0, s>>>(beta, p->n, (T*)dr, wbs);
  PreSlot slot(p, s);
  return mean_vjp_grad<T>(p->model, p->d, (const T*)p->Xt, p->N, (int)p->n, Xst, M, (int)m, theta, (const T*)p->alpha,
                          beta, (const T*)wts, (T*)(w + L.part), (T*)dtheta, s, bt, wbs, p->B > 1 ? p->ntheta : 0, p->pre, slot.staging);
}

// streamed period moments: the prediction's work area (its first stages leave V, Xs's SoA copy and the predicted variance
// there), then the moment pass's work area
template <typename T>
static int post_period(dgp_plan* p, const double* theta, const void* Xs, int64_t m, int mode, const void* mu, const double* scale2,
                       const double* w, const int32_t* group, int P, const void* ev, void* work, double* mean_out, double* cov_out,
                       hipStream_t s) {
  double* pm = (double*)((char*)work + predict_site_bytes(p, m) * (size_t)p->B);
  T *V, *Xst, *vpad;
  long wbs;
  // the latent mean the prediction also writes (B x m elements) lands in the moment pass's area, which its first launch resets
  int rc = predict_common<T>(p, theta, Xs, m, work, pm, &V, &Xst, &vpad, &wbs, s);
  if (rc) return rc;
  return posterior_period_moments<T>(mode, p->model, p->d, V, p->N, (long)m, p->B, Xst, vpad, wbs, theta, (const T*)mu, scale2, w,
                                     group, P, (const T*)ev, pm, mean_out, cov_out, s, p->pre);
}

// streamed exceedance moments: the prediction's work area as for post_period, one covariance panel of R x M elements per site,
// then the moment pass's work area
static size_t exceed_panel_bytes(const dgp_plan* p, int64_t m, int panel_rows) {
  return align_up(p->elem * (size_t)exceedance_panel_rows((long)m, panel_rows) * (size_t)round_up(m, DGP_TILE_HOST));
}
template <typename T>
static int post_exceed(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* mu, const double* thresh, int L,
                       const double* w, const int32_t* group, int P, const void* ev, int panel_rows, void* work, double* mean_out,
                       double* cov_out, hipStream_t s) {
  const size_t pb = exceed_panel_bytes(p, m, panel_rows);
  T* panel = (T*)((char*)work + predict_site_bytes(p, m) * (size_t)p->B);
  double* ex = (double*)((char*)panel + pb * (size_t)p->B);
  T *V, *Xst, *vpad;
  long wbs;
  // the latent mean the prediction also writes (B x m elements) lands in the moment pass's area, which its first launches reset
  int rc = predict_common<T>(p, theta, Xs, m, work, ex, &V, &Xst, &vpad, &wbs, s);
  if (rc) return rc;
  return posterior_exceedance_moments<T>(p->model, p->d, V, p->N, (long)m, p->B, Xst, vpad, wbs, theta, (const T*)mu, thresh, L, w, group,
                                         P, (const T*)ev, panel_rows, panel, (long)(pb / sizeof(T)), ex, mean_out, cov_out, s, p->pre);
}

// ---- posterior products of `planes` side-by-side cross Grams per test point: the covariance's additive parts (dgp_terms.hip,
// planes = C) and the value with its input derivatives (dgp_slopes.hip, planes = P = 1 + ncols).  Work area per site: the test
// points' SoA copy, the cross Grams side by side (N x planes M), V = T Ks of the same shape, `prior_rows` rows of M prior
// (co)variances -- the parts' C variances, or the derivatives' packed P (P + 1) / 2 block -- and the slab partials.
struct PlanesLayout {
  size_t Xst, Ks, V, prior, part, total;
};
static PlanesLayout planes_layout(const dgp_plan* p, int64_t m, int planes, int prior_rows) {
  const size_t M = (size_t)round_up(m, DGP_TILE_HOST), e = p->elem, N = (size_t)p->N;
  PlanesLayout L;
  size_t o = 0;
  L.Xst = o; o += align_up(e * M * p->d);
  L.Ks = o; o += align_up(e * N * (size_t)planes * M);
  L.V = o; o += align_up(e * N * (size_t)planes * M);
  L.prior = o; o += align_up(e * (size_t)prior_rows * M);
  L.part = o; o += align_up(e * (size_t)terms_partials(planes, (long)M));
  L.total = o;
  return L;
}

// The driver: pack the test points, fill the cross planes, the prior rows, V = T Ks at width planes x M, reduce.  The three
// launchers that differ between the products are callables:
//   cross(Xst, M, Ks, bt, wbs, staging)      prior(Xst, M, prior, wb, wbs)      reduce(V, Ks, M, prior, part, bt, wbs)
template <typename T, typename Cross, typename Prior, typename Reduce>
static int predict_planes(dgp_plan* p, const void* Xs, int64_t m, const PlanesLayout& L, int planes, void* work, hipStream_t s,
                          Cross cross, Prior prior, Reduce reduce) {
  const long M = round_up(m, DGP_TILE_HOST);
  const long wbs = p->B > 1 ? (long)(L.total / sizeof(T)) : 0;
  const Batch bt = batch_of<T>(p);
  char* w = (char*)work;
  T* Xst = (T*)(w + L.Xst);
  T* Ks = (T*)(w + L.Ks);
  T* V = (T*)(w + L.V);
  T* pr = (T*)(w + L.prior);
  Batch wb;  // the test points: [B][m][d] -> SoA in the work area
  wb.B = p->B;
  wb.ws = wbs;
  int rc = pack_x<T>((const T*)Xs, (int)m, p->d, M, Xst, s, wb);
  if (rc) return rc;
  {
    PreSlot slot(p, s);
    if ((rc = cross(Xst, M, Ks, bt, wbs, slot.staging))) return rc;
  }
  wb.ws = 0;
  if ((rc = prior(Xst, M, pr, wb, wbs))) return rc;
  if ((rc = predict_v<T>((const T*)p->Tm, p->N, Ks, (long)planes * M, V, s, bt, wbs))) return rc;
  return reduce(V, Ks, M, pr, (T*)(w + L.part), bt, wbs);
}

template <typename T>
static int predict_terms(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* mean, void* cov,
                         hipStream_t s) {
  const int C = model_nterms(p->model, p->d);
  return predict_planes<T>(
      p, Xs, m, planes_layout(p, m, C, C), C, work, s,
      [&](const T* Xst, long M, T* Ks, const Batch& bt, long wbs, void* staging) {
        return gram_cross_terms<T>(p->model, p->d, (const T*)p->Xt, p->N, (int)p->n, Xst, M, (int)m, theta, Ks, s, bt, wbs, p->pre, staging);
      },
      [&](const T* Xst, long M, T* kss, const Batch& wb, long wbs) {
        return gram_diag_terms<T>(p->model, p->d, Xst, M, (int)m, theta, kss, s, wb, wbs, p->pre);
      },
      [&](const T* V, const T* Ks, long M, const T* kss, T* part, const Batch& bt, long wbs) {
        return terms_reduce<T>(C, V, Ks, p->N, M, (int)m, (const T*)p->alpha, kss, part, (T*)mean, (T*)cov, s, bt, wbs);
      });
}

template <typename T>
static int predict_slopes(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const int* cols, int ncols, void* work,
                          void* mean, void* cov, hipStream_t s) {
  const int P = 1 + ncols;
  return predict_planes<T>(
      p, Xs, m, planes_layout(p, m, P, P * (P + 1) / 2), P, work, s,
      [&](const T* Xst, long M, T* Ks, const Batch& bt, long wbs, void* staging) {
        return gram_cross_slopes<T>(p->model, p->d, (const T*)p->Xt, p->N, (int)p->n, Xst, M, (int)m, theta, cols, ncols, Ks, s, bt, wbs,
                                    p->pre, staging);
      },
      [&](const T* Xst, long M, T* prior, const Batch& wb, long wbs) {
        return gram_prior_slopes<T>(p->model, p->d, Xst, M, (int)m, theta, cols, ncols, prior, s, wb, wbs, p->pre);
      },
      [&](const T* V, const T* Ks, long M, const T* prior, T* part, const Batch& bt, long wbs) {
        return slopes_reduce<T>(P, V, Ks, p->N, M, (int)m, (const T*)p->alpha, prior, part, (T*)mean, (T*)cov, s, bt, wbs);
      });
}

#define DGP_BY_DTYPE(p, CALL64, CALL32) ((p)->dtype == DGP_F64 ? (CALL64) : (CALL32))
#define DGP_CHECK_PLAN(p)                                                        \
  if (!(p)) return fail(DGP_E_ARG, "null plan");                                 \
  if (!(p)->ws) return fail(DGP_E_WORKSPACE, "plan has no workspace: call dgp_plan_set_workspace")
#define DGP_SINGLE_SITE(p) \
  if ((p)->B != 1)         \
  return fail(DGP_E_STATE, "batched plans support dgp_set_inputs / dgp_fit_step / dgp_factorize / dgp_predict / dgp_predict_mean / dgp_mean_vjp only")
static int wrap(int rc, const char* where) {
  if (rc > 0) return hipfail((hipError_t)rc, where);
  if (rc < 0) return fail(rc, where);
  return 0;
}

extern "C" {

int dgp_set_inputs(dgp_plan* p, const void* X, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!X) return fail(DGP_E_ARG, "dgp_set_inputs: null X");
  hipStream_t s = (hipStream_t)stream;
  int rc = DGP_BY_DTYPE(p, pack_x<double>((const double*)X, (int)p->n, p->d, p->N, (double*)p->Xt, s, batch_of<double>(p)),
                        pack_x<float>((const float*)X, (int)p->n, p->d, p->N, (float*)p->Xt, s, batch_of<float>(p)));
  p->have_inputs = 1;
  p->have_factor = 0;
  return wrap(rc, "dgp_set_inputs");
}

int dgp_fit_step(dgp_plan* p, const double* theta, const void* r, const void* noise, void* out, void* dr,
                 void* dnoise, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!theta || !r || !noise || !out) return fail(DGP_E_ARG, "dgp_fit_step: null argument");
  if (!p->have_inputs) return fail(DGP_E_STATE, "dgp_fit_step: call dgp_set_inputs first");
  hipStream_t s = (hipStream_t)stream;
  int rc = DGP_BY_DTYPE(p, fit_step<double>(p, theta, r, noise, out, dr, dnoise, 1, s),
                        fit_step<float>(p, theta, r, noise, out, dr, dnoise, 1, s));
  return wrap(rc, "dgp_fit_step");
}

int dgp_factorize(dgp_plan* p, const double* theta, const void* r, const void* noise, void* out, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!theta || !r || !noise || !out) return fail(DGP_E_ARG, "dgp_factorize: null argument");
  if (!p->have_inputs) return fail(DGP_E_STATE, "dgp_factorize: call dgp_set_inputs first");
  hipStream_t s = (hipStream_t)stream;
  int rc = DGP_BY_DTYPE(p, fit_step<double>(p, theta, r, noise, out, nullptr, nullptr, 0, s),
                        fit_step<float>(p, theta, r, noise, out, nullptr, nullptr, 0, s));
  return wrap(rc, "dgp_factorize");
}

}  // extern "C"

// ---- censored observations: Newton's mode search on the factorise path, then one step at the mode (dgp_censored.hip).
// One code path for a single-site plan and for a batch: every Newton iteration factorises ALL sites in lockstep; a site is done when
// it has no censored row, its proposal is within tol or its factorisation failed, and a done site is frozen on the device
// (CEN_ST_DONE), so that it rides through the remaining factorisations on unchanged pseudo-data.  The host reads the B status
// blocks in one copy per iteration.  stat: [B][4].  `batched`: the entry's texts name the site.
// Returns 0, a HIP error (> 0), or DGP_E_ARG / DGP_E_NOCONV with the error text already set.
static int laplace(dgp_plan* p, const double* theta, const double* y, const double* mean, const double* noise, const int* side,
                   double* f, int maxit, double tol, char* work, double* out, double* dr, double* stat, int with_grad, int batched,
                   const char* where, hipStream_t s, const double* upper = nullptr, int interval = 0) {
  const int B = p->B;
  const CensoredLayout L = censored_layout(p->N, p->n, B);
  const Batch bt = batch_of<double>(p);
  auto D = [&](size_t off) { return (double*)(work + off); };
  const int n = (int)p->n;
  const long wss = (long)(L.slice / sizeof(double));
  const double* alpha = (const double*)p->alpha;
  std::vector<double> st((size_t)B * CEN_ST_LEN);
  auto S = [&](int b, int k) -> double { return st[(size_t)b * CEN_ST_LEN + k]; };
  auto read_status = [&]() -> int {
    hipError_t e = hipMemcpyAsync(st.data(), D(L.status), sizeof(double) * st.size(), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return (int)e;
  };
  int rc;
  for (int k = 0; k < 4 * B; ++k) stat[k] = 0.0;
  if ((rc = censored_terms(f, y, side, noise, mean, n, 1, 0, work, L, s, bt, upper)) || (rc = read_status())) return rc;
  bool any = false, any_plain = false;
  for (int b = 0; b < B; ++b) {
    if (interval && S(b, CEN_ST_BAD) != 0.0) {
      snprintf(g_err, sizeof(g_err), upper ? "%s: side values must be -1, 0, +1 or 2 (site %d)"
                                           : "%s: a row of side 2 needs upper_dev; other side values must be -1, 0 or +1 (site %d)",
               where, b);
      return DGP_E_ARG;
    }
    if (S(b, CEN_ST_BADBRK) != 0.0) {
      snprintf(g_err, sizeof(g_err), "%s: %d bad bracket(s) in site %d: a row of side 2 needs a finite upper above its y", where,
               (int)S(b, CEN_ST_BADBRK), b);
      return DGP_E_ARG;
    }
    if (S(b, CEN_ST_BAD) != 0.0) {
      if (batched)
        snprintf(g_err, sizeof(g_err), "%s: side values must be -1, 0 or +1 (site %d)", where, b);
      else
        snprintf(g_err, sizeof(g_err), "%s: side values must be -1, 0 or +1", where);
      return DGP_E_ARG;
    }
    (S(b, CEN_ST_NCENS) != 0.0 ? any : any_plain) = true;
  }
  if (!any) {  // nothing censored: the plain step on (y - m, v), bit for bit
    if ((rc = fit_step<double>(p, theta, D(L.rt), D(L.nn), out, with_grad ? dr : nullptr, with_grad ? D(L.dnoise) : nullptr, with_grad, s)))
      return rc;
    return censored_mode(f, mean, alpha, n, work, L, s, bt);
  }
  if ((rc = (int)hipMemsetAsync(D(L.acur), 0, sizeof(double) * (size_t)B * (size_t)n, s))) return rc;
  std::vector<char> active((size_t)B);
  for (int b = 0; b < B; ++b) active[b] = S(b, CEN_ST_DONE) == 0.0;
  int it = 0;
  for (;;) {
    if ((rc = fit_step<double>(p, theta, D(L.rt), D(L.nn), D(L.out), nullptr, nullptr, 0, s))) return rc;
    ++it;
    // proposal, line search, update; then the next system (or the one at the mode) of every site that moved
    if ((rc = censored_newton_update(f, y, side, noise, mean, alpha, n, it, tol, work, L, s, bt, upper)) ||
        (rc = censored_terms(f, y, side, noise, mean, n, 0, it, work, L, s, bt, upper)) || (rc = read_status()))
      return rc;
    bool all_done = true;
    for (int b = 0; b < B; ++b) {
      if (!active[b]) continue;
      stat[4 * b] = (double)it;
      stat[4 * b + 1] = S(b, CEN_ST_DMAX);
      stat[4 * b + 2] += S(b, CEN_ST_HALVINGS);
      if (S(b, CEN_ST_DONE) != 0.0)
        active[b] = 0;  // converged, or not positive definite: f did not move; the step below reports it through DGP_OUT_INFO
      else
        all_done = false;
    }
    if (all_done || it >= maxit) break;
  }
  if ((rc = fit_step<double>(p, theta, D(L.rt), D(L.nn), out, nullptr, with_grad ? D(L.dnoise) : nullptr, with_grad, s))) return rc;
  if (with_grad) {
    if ((rc = censored_weights(alpha, n, p->N, work, L, s, bt))) return rc;
    // u = T^T (T w) in the work area: the plan's z, alpha and result rows stay as the step left them
    if ((rc = solve_work<double>((const double*)p->Tm, p->N, D(L.slices + L.w), n, D(L.slices + L.z), D(L.slices + L.u),
                                 D(L.slices + L.spart), D(L.slices + L.quad), wss, s, bt)))
      return rc;
    // (the step's Gram build left this theta in the plan's hyperparameter scratch)
    if ((rc = gram_bilinear<double>(p->model, p->d, (const double*)p->Xt, p->N, n, theta, D(L.slices + L.u), alpha,
                                    D(L.slices + L.gpart), out + DGP_OUT_DTHETA, 1, s, bt, wss, bt.ws, wss, DGP_OUT_LEN, p->pre, false,
                                    nullptr)))
      return rc;
  }
  if (any_plain && (rc = censored_mode(f, mean, alpha, n, work, L, s, bt))) return rc;  // the batch-mates without a censored row
  if ((rc = censored_result(alpha, side, (const double*)p->dr_w, n, with_grad, out, dr, work, L, s, bt)) || (rc = read_status())) return rc;
  int open_site = -1;
  for (int b = 0; b < B; ++b) {
    stat[4 * b + 3] = S(b, CEN_ST_CAPPED);
    if (active[b] && open_site < 0) open_site = b;
  }
  if (open_site >= 0) {
    if (batched)
      snprintf(g_err, sizeof(g_err), "%s: the mode search of site %d did not converge in %d Newton iterations (max |df| = %.3g)", where,
               open_site, it, stat[4 * open_site + 1]);
    else
      snprintf(g_err, sizeof(g_err), "%s: the mode search did not converge in %d Newton iterations (max |df| = %.3g)", where, it, stat[1]);
    return DGP_E_NOCONV;
  }
  return 0;
}
static int laplace_entry(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                         void* f, int maxit, double tol, void* work, size_t work_bytes, void* out, void* dr, double* stat,
                         int with_grad, int batched, const char* where, void* stream, const void* upper = nullptr, int interval = 0) {
  char msg[160];
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (batched ? p->dtype != DGP_F64 : (p->dtype != DGP_F64 || p->B != 1)) {
    if (batched)
      snprintf(msg, sizeof(msg), "%s: censored fits need a float64 plan (fp32 plans are not supported)", where);
    else
      snprintf(msg, sizeof(msg), "%s: censored fits need a float64 single-site plan (fp32 and batched plans are not supported)", where);
    return fail(DGP_E_ARG, msg);
  }
  if (!theta || !y || !mean || !noise || !side || !f || !out || !stat || maxit < 1 || !(tol >= 0.0)) {
    snprintf(msg, sizeof(msg), "%s: null argument (f_dev included), maxit < 1 or a negative tol", where);
    return fail(DGP_E_ARG, msg);
  }
  DGP_CHECK_PLAN(p);
  if (!p->have_inputs) return fail(DGP_E_STATE, "dgp_laplace_*: call dgp_set_inputs first");
  if (!work || work_bytes < (batched ? dgp_laplace_batched_workspace_bytes(p) : dgp_laplace_workspace_bytes(p))) {
    snprintf(msg, sizeof(msg), "%s: workspace missing or too small", where);
    return fail(DGP_E_WORKSPACE, msg);
  }
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_laplace_*: the work area must be 256-byte aligned");
  const int rc = laplace(p, theta, (const double*)y, (const double*)mean, (const double*)noise, (const int*)side, (double*)f, maxit, tol,
                         (char*)work, (double*)out, (double*)dr, stat, with_grad, batched, where, (hipStream_t)stream,
                         (const double*)upper, interval);
  if (rc == DGP_E_ARG || rc == DGP_E_NOCONV) return rc;  // text set where it arose
  return wrap(rc, where);
}

// ---- censored observations by expectation propagation (dgp_ep.hip): parallel sweeps on the factorise path, then (fit step) one
// step at the final sites, whose explicit gradient IS the gradient at the fixed point.  The host reads one status block per sweep.
// The sites that were factorised last are the result (a converged or last sweep's proposal is not applied), so the plan's
// factorisation, k, the cavities and log Z^ belong to one state.  stat: [6].
static int ep(dgp_plan* p, const double* theta, const double* y, const double* mean, const double* noise, const int* side,
              const double* upper, double* yt, double* nt, int cold, int maxit, double tol, double damping, char* work, double* out,
              double* dr, double* stat, double* cav_mean, double* cav_var, double* logz, int with_grad, const char* where, hipStream_t s) {
  const EpLayout L = ep_layout(p->N, p->n);
  const Batch bt = batch_of<double>(p);
  auto D = [&](size_t off) { return (double*)(work + off); };
  const int n = (int)p->n;
  const double* alpha = (const double*)p->alpha;
  const double* Tm = (const double*)p->Tm;
  double st[CEN_ST_LEN > EP_ST_LEN ? CEN_ST_LEN : EP_ST_LEN];
  auto read_status = [&](size_t off, int len) -> int {
    hipError_t e = hipMemcpyAsync(st, D(off), sizeof(double) * (size_t)len, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return (int)e;
  };
  int rc;
  for (int k = 0; k < 6; ++k) stat[k] = 0.0;
  // the Laplace terms at f = m: the rows are checked as the Laplace entries check them, and a cold start is their pseudo-data
  if ((rc = censored_terms(mean, y, side, noise, mean, n, 1, 0, work, L.cen, s, bt, upper)) || (rc = read_status(L.cen.status, CEN_ST_LEN)))
    return rc;
  if (st[CEN_ST_BAD] != 0.0) {
    snprintf(g_err, sizeof(g_err),
             upper ? "%s: side values must be -1, 0, +1 or 2" : "%s: a row of side 2 needs upper_dev; other side values must be -1, 0 or +1",
             where);
    return DGP_E_ARG;
  }
  if (st[CEN_ST_BADBRK] != 0.0) {
    snprintf(g_err, sizeof(g_err), "%s: %d bad bracket(s): a row of side 2 needs a finite upper above its y", where, (int)st[CEN_ST_BADBRK]);
    return DGP_E_ARG;
  }
  const double ncens = st[CEN_ST_NCENS];
  stat[5] = ncens;
  const bool aux = cav_mean || cav_var || logz;
  if (ncens == 0.0) {  // nothing censored: the plain step on (y - m, v), bit for bit; the sites are (y, v)
    if ((rc = fit_step<double>(p, theta, D(L.cen.rt), D(L.cen.nn), out, with_grad ? dr : nullptr, with_grad ? D(L.cen.dnoise) : nullptr,
                               with_grad, s)) ||
        (rc = ep_init(y, side, noise, mean, yt, nt, n, 1, work, L, s)))
      return rc;
    if (aux && ((rc = ep_diag(Tm, p->N, n, D(L.kdiag), work, L, s)) ||
                (rc = ep_result(alpha, y, side, noise, upper, yt, nt, n, nullptr, cav_mean, cav_var, logz, work, L, s))))
      return rc;
    return 0;
  }
  if ((rc = ep_init(y, side, noise, mean, yt, nt, n, cold, work, L, s))) return rc;
  int it = 0;
  bool conv = false;
  for (;;) {
    if ((rc = fit_step<double>(p, theta, D(L.cen.rt), nt, D(L.cen.out), nullptr, nullptr, 0, s))) return rc;
    ++it;
    if ((rc = ep_sweep(Tm, p->N, alpha, y, side, noise, mean, upper, yt, nt, n, it, it >= maxit, tol, damping, work, L, s)) ||
        (rc = read_status(L.status, EP_ST_LEN)))
      return rc;
    stat[0] = (double)it;
    stat[1] = st[EP_ST_DMU];
    stat[2] = st[EP_ST_DTAU];
    stat[3] = st[EP_ST_CAPPED];
    stat[4] = st[EP_ST_HELD];
    conv = st[EP_ST_DONE] != 0.0;  // converged, or not positive definite: the result row reports that through DGP_OUT_INFO
    if (conv || it >= maxit) break;
  }
  if (with_grad) {
    // the same system once more with K^^-1 and the gradient contraction: the same T and alpha, so k stays valid
    if ((rc = fit_step<double>(p, theta, D(L.cen.rt), nt, out, dr, D(L.cen.dnoise), 1, s))) return rc;
  } else if ((rc = (int)hipMemcpyAsync(out, D(L.cen.out), sizeof(double) * DGP_OUT_LEN, hipMemcpyDeviceToDevice, s))) {
    return rc;
  }
  if ((rc = ep_result(alpha, y, side, noise, upper, yt, nt, n, out, cav_mean, cav_var, logz, work, L, s)) || (rc = (int)hipStreamSynchronize(s)))
    return rc;
  if (!conv) {
    snprintf(g_err, sizeof(g_err), "%s: expectation propagation did not converge in %d sweeps (max |dmu| = %.3g, max v |dtau| = %.3g)",
             where, it, stat[1], stat[2]);
    return DGP_E_NOCONV;
  }
  return 0;
}
static int ep_entry(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                    const void* upper, void* yt, void* nt, int cold, int maxit, double tol, double damping, void* work, size_t work_bytes,
                    void* out, void* dr, double* stat, void* cav_mean, void* cav_var, void* logz, int with_grad, const char* where,
                    void* stream) {
  char msg[200];
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (p->dtype != DGP_F64 || p->B != 1) {
    snprintf(msg, sizeof(msg), "%s: expectation propagation needs a float64 single-site plan (fp32 and batched plans are not supported)", where);
    return fail(DGP_E_ARG, msg);
  }
  if (!theta || !y || !mean || !noise || !side || !yt || !nt || !out || !stat || maxit < 1 || !(tol >= 0.0)) {
    snprintf(msg, sizeof(msg), "%s: null argument (ytilde_dev / ntilde_dev included), maxit < 1 or a negative tol", where);
    return fail(DGP_E_ARG, msg);
  }
  if (!(damping > 0.0 && damping <= 1.0)) {
    snprintf(msg, sizeof(msg), "%s: damping must lie in (0, 1]", where);
    return fail(DGP_E_ARG, msg);
  }
  DGP_CHECK_PLAN(p);
  if (!p->have_inputs) return fail(DGP_E_STATE, "dgp_ep_*: call dgp_set_inputs first");
  if (!work || work_bytes < dgp_ep_workspace_bytes(p)) {
    snprintf(msg, sizeof(msg), "%s: workspace missing or too small", where);
    return fail(DGP_E_WORKSPACE, msg);
  }
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_ep_*: the work area must be 256-byte aligned");
  const int rc = ep(p, theta, (const double*)y, (const double*)mean, (const double*)noise, (const int*)side, (const double*)upper,
                    (double*)yt, (double*)nt, cold, maxit, tol, damping, (char*)work, (double*)out, (double*)dr, stat, (double*)cav_mean,
                    (double*)cav_var, (double*)logz, with_grad, where, (hipStream_t)stream);
  if (rc == DGP_E_ARG || rc == DGP_E_NOCONV) return rc;  // text set where it arose
  return wrap(rc, where);
}

extern "C" {

size_t dgp_ep_workspace_bytes(const dgp_plan* p) {
  if (!p || p->dtype != DGP_F64 || p->B != 1) return 0;
  return ep_layout(p->N, p->n).total;
}

int dgp_ep_fit_step(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                    const void* upper, void* ytilde, void* ntilde, int cold_start, int maxit, double tol, double damping, void* work,
                    size_t work_bytes, void* out, void* dr, double* stat, void* cav_mean, void* cav_var, void* logz, void* stream) {
  return ep_entry(p, theta, y, mean, noise, side, upper, ytilde, ntilde, cold_start, maxit, tol, damping, work, work_bytes, out, dr, stat,
                  cav_mean, cav_var, logz, 1, "dgp_ep_fit_step", stream);
}

int dgp_ep_factorize(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                     const void* upper, void* ytilde, void* ntilde, int cold_start, int maxit, double tol, double damping, void* work,
                     size_t work_bytes, void* out, double* stat, void* cav_mean, void* cav_var, void* logz, void* stream) {
  return ep_entry(p, theta, y, mean, noise, side, upper, ytilde, ntilde, cold_start, maxit, tol, damping, work, work_bytes, out, nullptr,
                  stat, cav_mean, cav_var, logz, 0, "dgp_ep_factorize", stream);
}

int dgp_ep_diag(dgp_plan* p, void* k, void* work, size_t work_bytes, void* stream) {
  if (!p || p->dtype != DGP_F64 || p->B != 1) return fail(DGP_E_ARG, "dgp_ep_diag: needs a float64 single-site plan");
  if (!k) return fail(DGP_E_ARG, "dgp_ep_diag: null argument");
  DGP_CHECK_PLAN(p);
  if (!p->have_factor) return fail(DGP_E_STATE, "dgp_ep_diag: no factorisation in the plan");
  if (!work || work_bytes < dgp_ep_workspace_bytes(p)) return fail(DGP_E_WORKSPACE, "dgp_ep_diag: workspace missing or too small");
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_ep_diag: the work area must be 256-byte aligned");
  return wrap(ep_diag((const double*)p->Tm, p->N, (int)p->n, (double*)k, (char*)work, ep_layout(p->N, p->n), (hipStream_t)stream),
              "dgp_ep_diag");
}

size_t dgp_laplace_workspace_bytes(const dgp_plan* p) {
  if (!p || p->dtype != DGP_F64 || p->B != 1) return 0;
  return censored_layout(p->N, p->n, 1).total;
}
size_t dgp_laplace_batched_workspace_bytes(const dgp_plan* p) {
  if (!p || p->dtype != DGP_F64) return 0;
  return censored_layout(p->N, p->n, p->B).total;
}

int dgp_laplace_fit_step(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                         void* f, int maxit, double tol, void* work, size_t work_bytes, void* out, void* dr, double* stat,
                         void* stream) {
  return laplace_entry(p, theta, y, mean, noise, side, f, maxit, tol, work, work_bytes, out, dr, stat, 1, 0, "dgp_laplace_fit_step",
                       stream);
}

int dgp_laplace_factorize(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                          void* f, int maxit, double tol, void* work, size_t work_bytes, void* out, double* stat, void* stream) {
  return laplace_entry(p, theta, y, mean, noise, side, f, maxit, tol, work, work_bytes, out, nullptr, stat, 0, 0, "dgp_laplace_factorize",
                       stream);
}

int dgp_laplace_batched_fit_step(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise,
                                 const int32_t* side, void* f, int maxit, double tol, void* work, size_t work_bytes, void* out, void* dr,
                                 double* stat, void* stream) {
  return laplace_entry(p, theta, y, mean, noise, side, f, maxit, tol, work, work_bytes, out, dr, stat, 1, 1,
                       "dgp_laplace_batched_fit_step", stream);
}

int dgp_laplace_batched_factorize(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise,
                                  const int32_t* side, void* f, int maxit, double tol, void* work, size_t work_bytes, void* out,
                                  double* stat, void* stream) {
  return laplace_entry(p, theta, y, mean, noise, side, f, maxit, tol, work, work_bytes, out, nullptr, stat, 0, 1,
                       "dgp_laplace_batched_factorize", stream);
}

int dgp_laplace_interval_fit_step(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise,
                                  const int32_t* side, const void* upper, void* f, int maxit, double tol, void* work, size_t work_bytes,
                                  void* out, void* dr, double* stat, void* stream) {
  return laplace_entry(p, theta, y, mean, noise, side, f, maxit, tol, work, work_bytes, out, dr, stat, 1, 1,
                       "dgp_laplace_interval_fit_step", stream, upper, 1);
}

int dgp_laplace_interval_factorize(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise,
                                   const int32_t* side, const void* upper, void* f, int maxit, double tol, void* work,
                                   size_t work_bytes, void* out, double* stat, void* stream) {
  return laplace_entry(p, theta, y, mean, noise, side, f, maxit, tol, work, work_bytes, out, nullptr, stat, 0, 1,
                       "dgp_laplace_interval_factorize", stream, upper, 1);
}

int dgp_debug_interval_terms(const double* za, const double* delta, int64_t count, double* out, void* stream) {
  if (!za || !delta || !out || count <= 0 || count > (1ll << 29))
    return fail(DGP_E_ARG, "dgp_debug_interval_terms: null argument / bad count");
  return wrap(debug_interval_terms(za, delta, count, out, (hipStream_t)stream), "dgp_debug_interval_terms");
}

int dgp_debug_censored_terms(const double* z, int64_t count, double* out, void* stream) {
  if (!z || !out || count <= 0 || count > (1ll << 29)) return fail(DGP_E_ARG, "dgp_debug_censored_terms: null argument / bad count");
  return wrap(debug_censored_terms(z, count, out, (hipStream_t)stream), "dgp_debug_censored_terms");
}

// u_dev / alpha_dev [B][n] -> dtheta_dev [B][ntheta]; B = 1: the single-site sweep
static int debug_bilinear(dgp_plan* p, const double* theta, const void* u, const void* alpha, void* work, size_t work_bytes, double* dtheta,
                          int batched, const char* where, void* stream) {
  char msg[160];
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (p->dtype != DGP_F64 || (!batched && p->B != 1)) {
    snprintf(msg, sizeof(msg), batched ? "%s: needs a float64 plan" : "%s: needs a float64 single-site plan", where);
    return fail(DGP_E_ARG, msg);
  }
  if (!theta || !u || !alpha || !dtheta) {
    snprintf(msg, sizeof(msg), "%s: null argument", where);
    return fail(DGP_E_ARG, msg);
  }
  DGP_CHECK_PLAN(p);
  if (!p->have_inputs) {
    snprintf(msg, sizeof(msg), "%s: call dgp_set_inputs first", where);
    return fail(DGP_E_STATE, msg);
  }
  if (!work || work_bytes < (batched ? dgp_laplace_batched_workspace_bytes(p) : dgp_laplace_workspace_bytes(p))) {
    snprintf(msg, sizeof(msg), "%s: workspace missing or too small", where);
    return fail(DGP_E_WORKSPACE, msg);
  }
  if (((uintptr_t)work & 255) != 0) {
    snprintf(msg, sizeof(msg), "%s: the work area must be 256-byte aligned", where);
    return fail(DGP_E_ARG, msg);
  }
  hipStream_t s = (hipStream_t)stream;
  const int B = p->B;
  const CensoredLayout L = censored_layout(p->N, p->n, B);
  char* slices = (char*)work + L.slices;
  double *up = (double*)(slices + L.u), *ap = (double*)(slices + L.w);
  const size_t nb = sizeof(double) * (size_t)p->n;
  hipError_t e = hipMemsetAsync(slices, 0, L.slice * (size_t)B, s);
  if (e == hipSuccess) e = hipMemcpy2DAsync(up, L.slice, u, nb, nb, (size_t)B, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemcpy2DAsync(ap, L.slice, alpha, nb, nb, (size_t)B, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return hipfail(e, where);
  const long wss = (long)(L.slice / sizeof(double));
  void* staging = p->pre ? p->ring.acquire(pre_scratch_bytes(B)) : nullptr;
  const int rc = gram_bilinear<double>(p->model, p->d, (const double*)p->Xt, p->N, (int)p->n, theta, up, ap, (double*)(slices + L.gpart),
                                       dtheta, 0, s, batch_of<double>(p), wss, wss, wss, p->ntheta, p->pre, true, staging);
  if (staging) p->ring.commit(s);
  p->pre_ready = 0;
  return wrap(rc, where);
}

int dgp_debug_bilinear(dgp_plan* p, const double* theta, const void* u, const void* alpha, void* work, size_t work_bytes, double* dtheta,
                       void* stream) {
  return debug_bilinear(p, theta, u, alpha, work, work_bytes, dtheta, 0, "dgp_debug_bilinear", stream);
}

int dgp_debug_bilinear_batched(dgp_plan* p, const double* theta, const void* u, const void* alpha, void* work, size_t work_bytes,
                               double* dtheta, void* stream) {
  return debug_bilinear(p, theta, u, alpha, work, work_bytes, dtheta, 1, "dgp_debug_bilinear_batched", stream);
}

size_t dgp_predict_workspace_bytes(const dgp_plan* p, int64_t m) {
  if (!p || m <= 0) return 0;
  return predict_site_bytes(p, m) * (size_t)p->B;
}

int dgp_predict(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, size_t work_bytes,
                void* mean, void* var, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!theta || !Xs || !work || !mean || !var || m <= 0) return fail(DGP_E_ARG, "dgp_predict: null argument");
  if (!p->have_factor) return fail(DGP_E_STATE, "dgp_predict: no factorisation in the plan (call dgp_factorize)");
  if (work_bytes < dgp_predict_workspace_bytes(p, m)) return fail(DGP_E_WORKSPACE, "dgp_predict: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = DGP_BY_DTYPE(p, predict<double>(p, theta, Xs, m, work, mean, var, s), predict<float>(p, theta, Xs, m, work, mean, var, s));
  return wrap(rc, "dgp_predict");
}

int dgp_posterior_cov(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, size_t work_bytes,
                      void* mean, void* cov, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!theta || !Xs || !work || !mean || !cov || m <= 0) return fail(DGP_E_ARG, "dgp_posterior_cov: null argument");
  if (!p->have_factor) return fail(DGP_E_STATE, "dgp_posterior_cov: no factorisation in the plan (call dgp_factorize)");
  if (work_bytes < dgp_predict_workspace_bytes(p, m)) return fail(DGP_E_WORKSPACE, "dgp_posterior_cov: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  int rc = DGP_BY_DTYPE(p, post_cov<double>(p, theta, Xs, m, work, mean, cov, s),
                        post_cov<float>(p, theta, Xs, m, work, mean, cov, s));
  return wrap(rc, "dgp_posterior_cov");
}

int dgp_model_nterms(int model, int d) { return model_nterms(model, d); }

size_t dgp_predict_terms_workspace_bytes(const dgp_plan* p, int64_t m) {
  if (!p || m <= 0) return 0;
  const int C = model_nterms(p->model, p->d);
  return planes_layout(p, m, C, C).total * (size_t)p->B;
}

int dgp_predict_terms(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, size_t work_bytes, void* mean,
                      void* cov, void* stream) {
  if (!p) return fail(DGP_E_ARG, "dgp_predict_terms: null plan");
  if (!theta || !Xs || !work || !mean || m <= 0) return fail(DGP_E_ARG, "dgp_predict_terms: null argument or m <= 0");
  if (!p->ws) return fail(DGP_E_WORKSPACE, "plan has no workspace: call dgp_plan_set_workspace");
  if (!p->have_factor) return fail(DGP_E_STATE, "dgp_predict_terms: no factorisation in the plan (call dgp_factorize)");
  if (work_bytes < dgp_predict_terms_workspace_bytes(p, m)) return fail(DGP_E_WORKSPACE, "dgp_predict_terms: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = DGP_BY_DTYPE(p, predict_terms<double>(p, theta, Xs, m, work, mean, cov, s),
                              predict_terms<float>(p, theta, Xs, m, work, mean, cov, s));
  return wrap(rc, "dgp_predict_terms");
}

int dgp_model_input_differentiable(int model, int d, int col) { return model_input_differentiable(model, d, col); }

size_t dgp_predict_slopes_workspace_bytes(const dgp_plan* p, int64_t m, int ncols) {
  if (!p || m <= 0 || ncols < 1 || ncols > p->d) return 0;
  const int P = 1 + ncols;
  return planes_layout(p, m, P, P * (P + 1) / 2).total * (size_t)p->B;
}

int dgp_predict_slopes(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const int* cols, int ncols, void* work,
                       size_t work_bytes, void* mean, void* cov, void* stream) {
  if (!p) return fail(DGP_E_ARG, "dgp_predict_slopes: null plan");
  if (!theta || !Xs || !cols || !work || !mean || m <= 0) return fail(DGP_E_ARG, "dgp_predict_slopes: null argument or m <= 0");
  if (ncols < 1 || ncols > p->d) return fail(DGP_E_ARG, "dgp_predict_slopes: ncols must be in 1 .. d");
  for (int q = 0; q < ncols; ++q) {
    if (cols[q] < 0 || cols[q] >= p->d) return fail(DGP_E_ARG, "dgp_predict_slopes: column outside 0 .. d - 1");
    for (int r = 0; r < q; ++r)
      if (cols[r] == cols[q]) return fail(DGP_E_ARG, "dgp_predict_slopes: repeated column");
  }
  for (int q = 0; q < ncols; ++q)
    if (model_input_differentiable(p->model, p->d, cols[q]) != 1)
      return fail(DGP_E_MODEL, "dgp_predict_slopes: the covariance is not differentiable in a requested column (Matern-1/2 factor)");
  if (!p->ws) return fail(DGP_E_WORKSPACE, "plan has no workspace: call dgp_plan_set_workspace");
  if (!p->have_factor) return fail(DGP_E_STATE, "dgp_predict_slopes: no factorisation in the plan (call dgp_factorize)");
  if (work_bytes < dgp_predict_slopes_workspace_bytes(p, m, ncols))
    return fail(DGP_E_WORKSPACE, "dgp_predict_slopes: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = DGP_BY_DTYPE(p, predict_slopes<double>(p, theta, Xs, m, cols, ncols, work, mean, cov, s),
                              predict_slopes<float>(p, theta, Xs, m, cols, ncols, work, mean, cov, s));
  return wrap(rc, "dgp_predict_slopes");
}

size_t dgp_mean_vjp_workspace_bytes(const dgp_plan* p, int64_t m) { return (p && m > 0) ? vjp_layout(p, m).total * (size_t)p->B : 0; }

int dgp_predict_mean(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, size_t work_bytes,
                     void* mean, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!theta || !Xs || !work || !mean || m <= 0) return fail(DGP_E_ARG, "dgp_predict_mean: null argument");
  if (!p->have_factor) return fail(DGP_E_STATE, "dgp_predict_mean: no factorisation in the plan");
  if (work_bytes < dgp_mean_vjp_workspace_bytes(p, m)) return fail(DGP_E_WORKSPACE, "dgp_predict_mean: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = DGP_BY_DTYPE(p, predict_mean<double>(p, theta, Xs, m, work, mean, s), predict_mean<float>(p, theta, Xs, m, work, mean, s));
  return wrap(rc, "dgp_predict_mean");
}

int dgp_mean_vjp(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* wts, void* work,
                 size_t work_bytes, void* dtheta, void* dr, void* dnoise, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!theta || !Xs || !wts || !work || !dtheta || m <= 0) return fail(DGP_E_ARG, "dgp_mean_vjp: null argument");
  if (!p->have_factor || !p->have_inverse)
    return fail(DGP_E_STATE, "dgp_mean_vjp: needs K^^-1 and alpha from dgp_fit_step at the same theta");
  if (work_bytes < dgp_mean_vjp_workspace_bytes(p, m)) return fail(DGP_E_WORKSPACE, "dgp_mean_vjp: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  return wrap(DGP_BY_DTYPE(p, mean_vjp<double>(p, theta, Xs, m, wts, work, dtheta, dr, dnoise, s),
                           mean_vjp<float>(p, theta, Xs, m, wts, work, dtheta, dr, dnoise, s)), "dgp_mean_vjp");
}

int dgp_sample_draws(int dtype, const void* L, int64_t m, const void* Z, int64_t ndraw, const void* mean, void* out,
                     void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_sample_draws: dtype must be 0 (f64) or 1 (f32)");
  if (!L || !Z || !out || m <= 0 || ndraw <= 0 || m > (1 << 20) || ndraw > (1 << 24))
    return fail(DGP_E_ARG, "dgp_sample_draws: null argument / bad size");
  const long M = round_up(m, DGP_TILE_HOST), Q = round_up(ndraw, DGP_TILE_HOST);
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == DGP_F64
                     ? sample_draws<double>((const double*)L, M, (const double*)Z, Q, (const double*)mean, (int)m, (int)ndraw, (double*)out, s)
                     : sample_draws<float>((const float*)L, M, (const float*)Z, Q, (const float*)mean, (int)m, (int)ndraw, (float*)out, s);
  return wrap(rc, "dgp_sample_draws");
}

size_t dgp_period_moments_workspace_bytes(int64_t m, int ngroups, int batch) {
  if (m <= 0 || m > (1 << 20) || ngroups <= 0 || ngroups > 65535 || batch <= 0 || batch > DGP_MAX_BATCH_SITES) return 0;
  return period_moments_workspace_bytes(m, ngroups, batch);
}

int dgp_period_moments(int dtype, int mode, const void* cov, int64_t m, int batch, const void* mu, const double* scale2,
                       const double* w, const int32_t* group, int ngroups, const void* extra_var, void* work,
                       size_t work_bytes, double* mean_out, double* cov_out, void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_period_moments: dtype must be 0 (f64) or 1 (f32)");
  if (mode != 0 && mode != 1) return fail(DGP_E_ARG, "dgp_period_moments: mode must be 0 (linear) or 1 (log)");
  if (!cov || !mu || !scale2 || !w || !group || !mean_out || !cov_out)
    return fail(DGP_E_ARG, "dgp_period_moments: null argument");
  if (m <= 0 || m > (1 << 20) || ngroups <= 0 || ngroups > 65535 || batch <= 0 || batch > DGP_MAX_BATCH_SITES)
    return fail(DGP_E_ARG, "dgp_period_moments: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= batch <= 1024)");
  if (!work || work_bytes < period_moments_workspace_bytes(m, ngroups, batch))
    return fail(DGP_E_WORKSPACE, "dgp_period_moments: workspace missing or too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == DGP_F64
                     ? period_moments<double>(mode, (const double*)cov, m, batch, (const double*)mu, scale2, w, group, ngroups,
                                              (const double*)extra_var, (double*)work, mean_out, cov_out, s)
                     : period_moments<float>(mode, (const float*)cov, m, batch, (const float*)mu, scale2, w, group, ngroups,
                                             (const float*)extra_var, (double*)work, mean_out, cov_out, s);
  return wrap(rc, "dgp_period_moments");
}

size_t dgp_posterior_period_moments_workspace_bytes(const dgp_plan* p, int64_t m, int ngroups) {
  if (!p || m <= 0 || m > (1 << 20) || ngroups <= 0 || ngroups > 65535) return 0;
  return predict_site_bytes(p, m) * (size_t)p->B + period_moments_workspace_bytes(m, ngroups, p->B);
}

int dgp_posterior_period_moments(dgp_plan* p, const double* theta, const void* Xs, int64_t m, int mode, const void* mu,
                                 const double* scale2, const double* w, const int32_t* group, int ngroups, const void* extra_var,
                                 void* work, size_t work_bytes, double* mean_out, double* cov_out, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (mode != 0 && mode != 1) return fail(DGP_E_ARG, "dgp_posterior_period_moments: mode must be 0 (linear) or 1 (log)");
  if (!theta || !Xs || !mu || !scale2 || !w || !group || !mean_out || !cov_out)
    return fail(DGP_E_ARG, "dgp_posterior_period_moments: null argument");
  if (m <= 0 || m > (1 << 20) || ngroups <= 0 || ngroups > 65535)
    return fail(DGP_E_ARG, "dgp_posterior_period_moments: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535)");
  if (!p->have_factor) return fail(DGP_E_STATE, "dgp_posterior_period_moments: no factorisation in the plan (call dgp_factorize)");
  DGP_CHECK_PLAN(p);
  if (!work || work_bytes < dgp_posterior_period_moments_workspace_bytes(p, m, ngroups))
    return fail(DGP_E_WORKSPACE, "dgp_posterior_period_moments: workspace missing or too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = DGP_BY_DTYPE(p, post_period<double>(p, theta, Xs, m, mode, mu, scale2, w, group, ngroups, extra_var, work, mean_out, cov_out, s),
                              post_period<float>(p, theta, Xs, m, mode, mu, scale2, w, group, ngroups, extra_var, work, mean_out, cov_out, s));
  return wrap(rc, "dgp_posterior_period_moments");
}

static bool wm_sizes_ok(int64_t m, int64_t q, int batch) {
  return m > 0 && m <= (1 << 20) && q > 0 && q <= (1 << 20) && batch > 0 && batch <= DGP_MAX_BATCH_SITES;
}
size_t dgp_window_moments_workspace_bytes(int64_t m, int64_t q, int batch) {
  if (!wm_sizes_ok(m, q, batch)) return 0;
  return window_moments_workspace_bytes(m, q, batch);
}

int dgp_window_moments(int dtype, int mode, const void* cov, int64_t m, int batch, const void* mu, const double* scale2,
                       const double* a, const int32_t* lo, const int32_t* hi, int64_t q, void* work, size_t work_bytes,
                       double* mean_out, double* cov_out, void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_window_moments: dtype must be 0 (f64) or 1 (f32)");
  if (mode != 0 && mode != 1) return fail(DGP_E_ARG, "dgp_window_moments: mode must be 0 (linear) or 1 (log)");
  if (!cov || !mu || !lo || !hi || !mean_out || !cov_out || (mode == 1 && !scale2))
    return fail(DGP_E_ARG, "dgp_window_moments: null argument");
  if (!wm_sizes_ok(m, q, batch))
    return fail(DGP_E_ARG, "dgp_window_moments: bad size (1 <= m <= 2^20, 1 <= q <= 2^20, 1 <= batch <= 1024)");
  if (!work || work_bytes < window_moments_workspace_bytes(m, q, batch))
    return fail(DGP_E_WORKSPACE, "dgp_window_moments: workspace missing or too small");
  if (((uintptr_t)work & 7) != 0) return fail(DGP_E_ARG, "dgp_window_moments: the work area must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == DGP_F64 ? window_moments<double>(mode, (const double*)cov, m, batch, (const double*)mu, scale2, a, lo, hi, q,
                                                           (double*)work, mean_out, cov_out, s)
                                  : window_moments<float>(mode, (const float*)cov, m, batch, (const float*)mu, scale2, a, lo, hi, q,
                                                          (double*)work, mean_out, cov_out, s);
  return wrap(rc, "dgp_window_moments");
}

static bool ex_sizes_ok(int64_t m, int ngroups, int nlevels, int batch) {
  return m > 0 && m <= (1 << 20) && ngroups > 0 && ngroups <= 65535 && nlevels >= 1 && nlevels <= 64 && batch > 0 &&
         batch <= DGP_MAX_BATCH_SITES;
}
size_t dgp_exceedance_moments_workspace_bytes(int64_t m, int ngroups, int nlevels, int batch) {
  if (!ex_sizes_ok(m, ngroups, nlevels, batch)) return 0;
  return exceedance_moments_workspace_bytes(m, ngroups, nlevels, batch);
}

int dgp_exceedance_moments(int dtype, const void* cov, int64_t m, int batch, const void* mu, const double* thresh, int nlevels,
                           const double* w, const int32_t* group, int ngroups, const void* extra_var, void* work,
                           size_t work_bytes, double* mean_out, double* cov_out, void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_exceedance_moments: dtype must be 0 (f64) or 1 (f32)");
  if (!cov || !mu || !thresh || !w || !group || !mean_out || !cov_out)
    return fail(DGP_E_ARG, "dgp_exceedance_moments: null argument");
  if (!ex_sizes_ok(m, ngroups, nlevels, batch))
    return fail(DGP_E_ARG,
                "dgp_exceedance_moments: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= nlevels <= 64, 1 <= batch <= 1024)");
  if (!work || work_bytes < exceedance_moments_workspace_bytes(m, ngroups, nlevels, batch))
    return fail(DGP_E_WORKSPACE, "dgp_exceedance_moments: workspace missing or too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == DGP_F64
                     ? exceedance_moments<double>((const double*)cov, m, batch, (const double*)mu, thresh, nlevels, w, group, ngroups,
                                                  (const double*)extra_var, (double*)work, mean_out, cov_out, s)
                     : exceedance_moments<float>((const float*)cov, m, batch, (const float*)mu, thresh, nlevels, w, group, ngroups,
                                                 (const float*)extra_var, (double*)work, mean_out, cov_out, s);
  return wrap(rc, "dgp_exceedance_moments");
}

size_t dgp_posterior_exceedance_moments_workspace_bytes(const dgp_plan* p, int64_t m, int ngroups, int nlevels, int panel_rows) {
  if (!p || !ex_sizes_ok(m, ngroups, nlevels, p->B) || panel_rows <= 0 || panel_rows % DGP_TILE_HOST != 0) return 0;
  return (predict_site_bytes(p, m) + exceed_panel_bytes(p, m, panel_rows)) * (size_t)p->B +
         exceedance_moments_workspace_bytes(m, ngroups, nlevels, p->B);
}

int dgp_posterior_exceedance_moments(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* mu, const double* thresh,
                                     int nlevels, const double* w, const int32_t* group, int ngroups, const void* extra_var,
                                     int panel_rows, void* work, size_t work_bytes, double* mean_out, double* cov_out, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!theta || !Xs || !mu || !thresh || !w || !group || !mean_out || !cov_out)
    return fail(DGP_E_ARG, "dgp_posterior_exceedance_moments: null argument");
  if (!ex_sizes_ok(m, ngroups, nlevels, p->B))
    return fail(DGP_E_ARG, "dgp_posterior_exceedance_moments: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= nlevels <= 64)");
  if (panel_rows <= 0 || panel_rows % DGP_TILE_HOST != 0)
    return fail(DGP_E_ARG, "dgp_posterior_exceedance_moments: panel_rows must be a positive multiple of 128");
  if (!p->have_factor)
    return fail(DGP_E_STATE, "dgp_posterior_exceedance_moments: no factorisation in the plan (call dgp_factorize or dgp_fit_step)");
  DGP_CHECK_PLAN(p);
  if (!work || work_bytes < dgp_posterior_exceedance_moments_workspace_bytes(p, m, ngroups, nlevels, panel_rows))
    return fail(DGP_E_WORKSPACE, "dgp_posterior_exceedance_moments: workspace missing or too small");
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_posterior_exceedance_moments: the work area must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  {  // a failed factorisation leaves no T to read: the sites' status words, before any launch
    std::vector<int> info((size_t)p->B, 0);
    hipError_t e = hipMemcpy2DAsync(info.data(), sizeof(int), p->info, p->site_bytes, sizeof(int), (size_t)p->B, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hipfail(e, "dgp_posterior_exceedance_moments");
    for (int b = 0; b < p->B; ++b)
      if (info[(size_t)b] != 0)
        return fail(DGP_E_STATE, "dgp_posterior_exceedance_moments: the factorisation the plan holds failed (matrix not positive definite)");
  }
  const int rc = DGP_BY_DTYPE(p, post_exceed<double>(p, theta, Xs, m, mu, thresh, nlevels, w, group, ngroups, extra_var, panel_rows, work, mean_out, cov_out, s),
                              post_exceed<float>(p, theta, Xs, m, mu, thresh, nlevels, w, group, ngroups, extra_var, panel_rows, work, mean_out, cov_out, s));
  return wrap(rc, "dgp_posterior_exceedance_moments");
}

static bool sv_sizes_ok(int64_t m, int ngroups, int nrows, int nterms, int batch) {
  return m > 0 && m <= (1 << 20) && ngroups > 0 && ngroups <= 65535 && nrows >= 0 && nrows <= 64 && nterms >= 1 && nterms <= 64 &&
         batch > 0 && batch <= DGP_MAX_BATCH_SITES;
}
size_t dgp_sample_value_workspace_bytes(int64_t m, int ngroups, int nrows, int nterms, int batch) {
  if (!sv_sizes_ok(m, ngroups, nrows, nterms, batch)) return 0;
  return sample_value_workspace_bytes(m, ngroups, nterms, batch);
}

int dgp_sample_value(int dtype, const void* cov, int64_t m, int batch, const double* a, const double* scale2, const int32_t* group,
                     int ngroups, const void* obs_var, const double* rows, int nrows, int nterms, void* work, size_t work_bytes,
                     double* gain_out, double* var_out, void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_sample_value: dtype must be 0 (f64) or 1 (f32)");
  if (!cov || !a || !scale2 || !group || !gain_out || !var_out) return fail(DGP_E_ARG, "dgp_sample_value: null argument");
  if (!sv_sizes_ok(m, ngroups, nrows, nterms, batch))
    return fail(DGP_E_ARG,
                "dgp_sample_value: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 0 <= nrows <= 64, 1 <= nterms <= 64, "
                "1 <= batch <= 1024)");
  if (nrows > 0 && !rows) return fail(DGP_E_ARG, "dgp_sample_value: null argument (rows with nrows > 0)");
  if (!work || work_bytes < sample_value_workspace_bytes(m, ngroups, nterms, batch))
    return fail(DGP_E_WORKSPACE, "dgp_sample_value: workspace missing or too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == DGP_F64 ? sample_value<double>((const double*)cov, m, batch, a, scale2, group, ngroups, (const double*)obs_var,
                                                         rows, nrows, nterms, (double*)work, gain_out, var_out, s)
                                  : sample_value<float>((const float*)cov, m, batch, a, scale2, group, ngroups, (const float*)obs_var,
                                                        rows, nrows, nterms, (double*)work, gain_out, var_out, s);
  return wrap(rc, "dgp_sample_value");
}

int dgp_debug_bvn_excess(const double* h, const double* k, const double* rho, int64_t count, double* out, void* stream) {
  if (!h || !k || !rho || !out || count <= 0 || count > (1ll << 31))
    return fail(DGP_E_ARG, "dgp_debug_bvn_excess: null argument / bad count");
  return wrap(debug_bvn_excess(h, k, rho, count, out, (hipStream_t)stream), "dgp_debug_bvn_excess");
}

static bool cv_sizes_ok(const dgp_plan* p, int ngroups, int64_t max_group) {
  return p && ngroups >= 1 && ngroups <= p->n && max_group >= 1 && max_group <= p->n;
}
size_t dgp_cross_validate_workspace_bytes(const dgp_plan* p, int ngroups, int64_t max_group) {
  if (!cv_sizes_ok(p, ngroups, max_group)) return 0;
  return cross_validate_workspace_bytes(p->N, p->B, ngroups, max_group);
}

int dgp_cross_validate(dgp_plan* p, const int32_t* order, const int32_t* start, int ngroups, int64_t max_group, void* work,
                       size_t work_bytes, double* resid, double* var, double* lpd, int32_t* info, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!order || !start || !resid || !var || !lpd || !info) return fail(DGP_E_ARG, "dgp_cross_validate: null argument");
  if (!cv_sizes_ok(p, ngroups, max_group))
    return fail(DGP_E_ARG, "dgp_cross_validate: bad size (1 <= ngroups <= n, 1 <= max_group <= n)");
  DGP_CHECK_PLAN(p);
  if (!p->have_factor) return fail(DGP_E_STATE, "dgp_cross_validate: no factorisation in the plan (call dgp_factorize or dgp_fit_step)");
  if (!work || work_bytes < dgp_cross_validate_workspace_bytes(p, ngroups, max_group))
    return fail(DGP_E_WORKSPACE, "dgp_cross_validate: workspace missing or too small");
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_cross_validate: the work area must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  // K^^-1 (S) is read when the last step left it valid and never written; after a bare dgp_factorize it is dead and ignored
  const void* S = p->have_inverse ? p->S : nullptr;
  const int rc = DGP_BY_DTYPE(
      p,
      cross_validate<double>((const double*)p->Tm, (const double*)S, (const double*)p->alpha, p->N, (int)p->n, order, start, ngroups,
                             max_group, work, resid, var, lpd, info, s, batch_of<double>(p)),
      cross_validate<float>((const float*)p->Tm, (const float*)S, (const float*)p->alpha, p->N, (int)p->n, order, start, ngroups, max_group,
                            work, resid, var, lpd, info, s, batch_of<float>(p)));
  return wrap(rc, "dgp_cross_validate");
}

static bool lcv_plan_ok(const dgp_plan* p) { return p && p->dtype == DGP_F64 && p->B == 1; }
size_t dgp_laplace_cross_validate_workspace_bytes(const dgp_plan* p, int ngroups, int64_t max_group) {
  if (!lcv_plan_ok(p) || !cv_sizes_ok(p, ngroups, max_group)) return 0;
  return laplace_cv_layout(p->N, p->n, ngroups, max_group).total;
}

int dgp_laplace_cross_validate(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                               const void* upper, const void* f, const int32_t* order, const int32_t* start, int ngroups,
                               int64_t max_group, double shift, void* work, size_t work_bytes, double* out, int32_t* info, void* stream) {
  const char* where = "dgp_laplace_cross_validate";
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!lcv_plan_ok(p))
    return fail(DGP_E_ARG, "dgp_laplace_cross_validate: needs a float64 single-site plan (fp32 and batched plans are not supported)");
  if (!theta || !y || !mean || !noise || !side || !f || !order || !start || !out || !info || !(shift == shift))
    return fail(DGP_E_ARG, "dgp_laplace_cross_validate: null argument (f_dev included) or a NaN shift");
  if (!cv_sizes_ok(p, ngroups, max_group))
    return fail(DGP_E_ARG, "dgp_laplace_cross_validate: bad size (1 <= ngroups <= n, 1 <= max_group <= n)");
  DGP_CHECK_PLAN(p);
  if (!p->have_factor)
    return fail(DGP_E_STATE, "dgp_laplace_cross_validate: no factorisation in the plan (call dgp_laplace_factorize or dgp_laplace_fit_step)");
  if (!work || work_bytes < dgp_laplace_cross_validate_workspace_bytes(p, ngroups, max_group))
    return fail(DGP_E_WORKSPACE, "dgp_laplace_cross_validate: workspace missing or too small");
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_laplace_cross_validate: the work area must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const LaplaceCvLayout L = laplace_cv_layout(p->N, p->n, ngroups, max_group);
  // the terms pass and its read-back first: the staging slot below is not held across the synchronisation
  int rc = laplace_cv_terms(p->N, (int)p->n, (const double*)y, (const double*)mean, (const double*)noise, side, (const double*)upper,
                            (const double*)f, (char*)work, L, s);
  if (rc == 0) {
    PreSlot slot(p, s);
    rc = laplace_cross_validate(p->model, p->d, (const double*)p->Xt, (const double*)p->Tm, (const double*)p->alpha, p->N, (int)p->n, theta,
                                (const double*)y, (const double*)noise, side, (const double*)upper, (const double*)f, order, start,
                                ngroups, shift, (char*)work, L, out, info, s, batch_of<double>(p), p->pre, slot.staging);
  }
  if (rc == LCV_E_SIDE_NO_UPPER)
    return fail(DGP_E_ARG, "dgp_laplace_cross_validate: a row of side 2 needs upper_dev; other side values must be -1, 0 or +1");
  if (rc == LCV_E_SIDE) return fail(DGP_E_ARG, "dgp_laplace_cross_validate: side values must be -1, 0, +1 or 2");
  if (rc == LCV_E_BRACKET)
    return fail(DGP_E_ARG, "dgp_laplace_cross_validate: bad bracket(s): a row of side 2 needs a finite upper above its y");
  return wrap(rc, where);
}

#define DGP_FISHER_MAX_DIAG 8
size_t dgp_fisher_workspace_bytes(const dgp_plan* p, int ndiag) {
  if (!p || ndiag < 0 || ndiag > DGP_FISHER_MAX_DIAG) return 0;
  return fisher_site_bytes(p->N, p->ntheta + ndiag, p->elem) * (size_t)p->B;
}

int dgp_fisher(dgp_plan* p, const double* theta, const void* diag, int ndiag, void* work, size_t work_bytes, double* fisher_out,
               void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!theta || !fisher_out) return fail(DGP_E_ARG, "dgp_fisher: null argument");
  if (ndiag < 0 || ndiag > DGP_FISHER_MAX_DIAG) return fail(DGP_E_ARG, "dgp_fisher: ndiag must be 0..8");
  if (ndiag > 0 && !diag) return fail(DGP_E_ARG, "dgp_fisher: ndiag > 0 needs the diagonal directions");
  DGP_CHECK_PLAN(p);
  if (!p->have_factor) return fail(DGP_E_STATE, "dgp_fisher: no factorisation in the plan (call dgp_factorize or dgp_fit_step)");
  if (!work || work_bytes < dgp_fisher_workspace_bytes(p, ndiag)) return fail(DGP_E_WORKSPACE, "dgp_fisher: workspace missing or too small");
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_fisher: the work area must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  {  // a failed factorisation leaves no T to read: the sites' status words, before any launch
    std::vector<int> info((size_t)p->B, 0);
    hipError_t e = hipMemcpy2DAsync(info.data(), sizeof(int), p->info, p->site_bytes, sizeof(int), (size_t)p->B, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hipfail(e, "dgp_fisher");
    for (int b = 0; b < p->B; ++b)
      if (info[(size_t)b] != 0) return fail(DGP_E_STATE, "dgp_fisher: the factorisation the plan holds failed (matrix not positive definite)");
  }
  PreSlot slot(p, s);
  const int rc = DGP_BY_DTYPE(
      p,
      fisher<double>(p->model, p->d, (const double*)p->Xt, (const double*)p->Tm, p->N, (int)p->n, theta, (const double*)diag, ndiag, work,
                     fisher_out, s, batch_of<double>(p), p->pre, slot.staging),
      fisher<float>(p->model, p->d, (const float*)p->Xt, (const float*)p->Tm, p->N, (int)p->n, theta, (const float*)diag, ndiag, work,
                    fisher_out, s, batch_of<float>(p), p->pre, slot.staging));
  return wrap(rc, "dgp_fisher");
}

}  // extern "C"

#define DGP_SENS_MAX_COLS 8
static bool sens_sizes_ok(const dgp_plan* p, int64_t m, int ndiag, int nrhs) {
  return p && m > 0 && m <= 0x7fffffffLL - DGP_TILE_HOST && ndiag >= 0 && ndiag <= DGP_SENS_MAX_COLS && nrhs >= 0 && nrhs <= DGP_SENS_MAX_COLS;
}
template <typename T>
static int sensitivity(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* diag, int ndiag, const void* rhs, int nrhs,
                       void* work, double* dmean, double* dvar, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST);
  const SensLayout L = sens_layout(p->N, M, p->d, p->ntheta, ndiag, nrhs, p->elem);
  char* w = (char*)work;
  const int rc = cross<T>(p, theta, Xs, m, w + L.Xst, w + L.Ks, s, (long)(L.total / sizeof(T)));
  if (rc) return rc;
  return predict_sensitivity<T>(p->model, p->d, (const T*)p->Xt, (const T*)p->Tm, (const T*)p->alpha, p->N, (int)p->n, theta, M, (int)m,
                                (const T*)diag, ndiag, (const T*)rhs, nrhs, work, L, dmean, dvar, s, batch_of<T>(p), p->pre);
}

extern "C" {

size_t dgp_predict_sensitivity_workspace_bytes(const dgp_plan* p, int64_t m, int ndiag, int nrhs) {
  if (!sens_sizes_ok(p, m, ndiag, nrhs)) return 0;
  return sens_layout(p->N, round_up(m, DGP_TILE_HOST), p->d, p->ntheta, ndiag, nrhs, p->elem).total * (size_t)p->B;
}

int dgp_predict_sensitivity(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* diag, int ndiag, const void* rhs,
                            int nrhs, void* work, size_t work_bytes, double* dmean, double* dvar, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!theta || !Xs || !dmean) return fail(DGP_E_ARG, "dgp_predict_sensitivity: null argument");
  if (m <= 0 || m > 0x7fffffffLL - DGP_TILE_HOST) return fail(DGP_E_ARG, "dgp_predict_sensitivity: m must be positive");
  if (ndiag < 0 || ndiag > DGP_SENS_MAX_COLS) return fail(DGP_E_ARG, "dgp_predict_sensitivity: ndiag must be 0..8");
  if (nrhs < 0 || nrhs > DGP_SENS_MAX_COLS) return fail(DGP_E_ARG, "dgp_predict_sensitivity: nrhs must be 0..8");
  if (ndiag > 0 && !diag) return fail(DGP_E_ARG, "dgp_predict_sensitivity: ndiag > 0 needs the diagonal directions");
  if (nrhs > 0 && !rhs) return fail(DGP_E_ARG, "dgp_predict_sensitivity: nrhs > 0 needs the right-hand-side columns");
  DGP_CHECK_PLAN(p);
  if (!p->have_factor)
    return fail(DGP_E_STATE, "dgp_predict_sensitivity: no factorisation in the plan (call dgp_factorize or dgp_fit_step)");
  if (!work || work_bytes < dgp_predict_sensitivity_workspace_bytes(p, m, ndiag, nrhs))
    return fail(DGP_E_WORKSPACE, "dgp_predict_sensitivity: workspace missing or too small");
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_predict_sensitivity: the work area must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  {  // a failed factorisation leaves no T to read: the sites' status words, before any launch
    std::vector<int> info((size_t)p->B, 0);
    hipError_t e = hipMemcpy2DAsync(info.data(), sizeof(int), p->info, p->site_bytes, sizeof(int), (size_t)p->B, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hipfail(e, "dgp_predict_sensitivity");
    for (int b = 0; b < p->B; ++b)
      if (info[(size_t)b] != 0)
        return fail(DGP_E_STATE, "dgp_predict_sensitivity: the factorisation the plan holds failed (matrix not positive definite)");
  }
  const int rc = DGP_BY_DTYPE(p, sensitivity<double>(p, theta, Xs, m, diag, ndiag, rhs, nrhs, work, dmean, dvar, s),
                              sensitivity<float>(p, theta, Xs, m, diag, ndiag, rhs, nrhs, work, dmean, dvar, s));
  return wrap(rc, "dgp_predict_sensitivity");
}

}  // extern "C"

static bool influence_sizes_ok(const dgp_plan* p, int64_t m, int nfolds, int64_t max_fold, int ngroups) {
  return p && m >= 1 && m <= (1 << 20) && nfolds >= 1 && nfolds <= p->n && max_fold >= 1 && max_fold <= p->n && ngroups >= 1 &&
         ngroups <= 65535;
}
static InfluenceLayout influence_layout_of(const dgp_plan* p, int64_t m, int nfolds, int64_t max_fold, int ngroups) {
  return influence_layout(p->N, p->B, (int)p->n, p->d, round_up(m, DGP_TILE_HOST), (int)m, nfolds, max_fold, ngroups, p->elem);
}
template <typename T>
static int influence(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const int32_t* order, const int32_t* start, int nfolds,
                     int64_t max_fold, int mode, const double* a, const double* scale, const int32_t* group, int ngroups,
                     const double* inv_sd, void* work, double* dload, double* dvar, double* shift, int32_t* info, hipStream_t s) {
  const InfluenceLayout L = influence_layout_of(p, m, nfolds, max_fold, ngroups);
  char* w = (char*)work;
  const int rc = cross<T>(p, theta, Xs, m, w + L.Xst, w + L.Ks, s, (long)(L.slice / sizeof(T)));
  if (rc) return rc;
  const void* S = p->have_inverse ? p->S : nullptr;  // as dgp_cross_validate: read when the last step left it valid
  return deletion_influence<T>((const T*)p->Tm, (const T*)S, (const T*)p->alpha, p->N, (int)p->n, round_up(m, DGP_TILE_HOST), (int)m, order,
                               start, nfolds, max_fold, mode, a, scale, group, ngroups, inv_sd, work, L, dload, dvar, shift, info, s,
                               batch_of<T>(p));
}

extern "C" {

size_t dgp_deletion_influence_workspace_bytes(const dgp_plan* p, int64_t m, int nfolds, int64_t max_fold, int ngroups) {
  if (!influence_sizes_ok(p, m, nfolds, max_fold, ngroups)) return 0;
  return influence_layout_of(p, m, nfolds, max_fold, ngroups).total;
}

int dgp_deletion_influence(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const int32_t* order, const int32_t* start,
                           int nfolds, int64_t max_fold, int mode, const double* a, const double* scale, const int32_t* group, int ngroups,
                           const double* inv_sd, void* work, size_t work_bytes, double* dload, double* dvar, double* shift,
                           int32_t* info, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!theta || !Xs || !order || !start || !a || !scale || !group || !dload || !info)
    return fail(DGP_E_ARG, "dgp_deletion_influence: null argument");
  if (!influence_sizes_ok(p, m, nfolds, max_fold, ngroups))
    return fail(DGP_E_ARG, "dgp_deletion_influence: bad size (1 <= m <= 2^20, 1 <= nfolds <= n, 1 <= max_fold <= n, 1 <= ngroups <= 65535)");
  if (mode != 0 && mode != 1) return fail(DGP_E_ARG, "dgp_deletion_influence: mode must be 0 (linear) or 1 (log)");
  if (mode == 1 && dvar) return fail(DGP_E_ARG, "dgp_deletion_influence: the variance change is exact for mode 0 only (dvar_dev must be NULL)");
  if (shift && !inv_sd) return fail(DGP_E_ARG, "dgp_deletion_influence: shift_dev needs inv_sd_dev");
  DGP_CHECK_PLAN(p);
  if (!p->have_factor) return fail(DGP_E_STATE, "dgp_deletion_influence: no factorisation in the plan (call dgp_factorize or dgp_fit_step)");
  if (!work || work_bytes < dgp_deletion_influence_workspace_bytes(p, m, nfolds, max_fold, ngroups))
    return fail(DGP_E_WORKSPACE, "dgp_deletion_influence: workspace missing or too small");
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_deletion_influence: the work area must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  {  // a failed factorisation leaves no T to read: the sites' status words, before any launch
    std::vector<int> st((size_t)p->B, 0);
    hipError_t e = hipMemcpy2DAsync(st.data(), sizeof(int), p->info, p->site_bytes, sizeof(int), (size_t)p->B, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hipfail(e, "dgp_deletion_influence");
    for (int b = 0; b < p->B; ++b)
      if (st[(size_t)b] != 0)
        return fail(DGP_E_STATE, "dgp_deletion_influence: the factorisation the plan holds failed (matrix not positive definite)");
  }
  const int rc = DGP_BY_DTYPE(p,
                              influence<double>(p, theta, Xs, m, order, start, nfolds, max_fold, mode, a, scale, group, ngroups, inv_sd, work,
                                                dload, dvar, shift, info, s),
                              influence<float>(p, theta, Xs, m, order, start, nfolds, max_fold, mode, a, scale, group, ngroups, inv_sd, work,
                                               dload, dvar, shift, info, s));
  return wrap(rc, "dgp_deletion_influence");
}

int dgp_plan_set_timing(dgp_plan* p, int enabled) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  p->timing = enabled ? 1 : 0;
  p->timed_valid = 0;
  return 0;
}

int dgp_plan_get_timing(dgp_plan* p, double* ms_out) {
  if (!p || !ms_out) return fail(DGP_E_ARG, "dgp_plan_get_timing: null argument");
  if (!p->timing || !p->tev || !p->timed_valid)
    return fail(DGP_E_STATE, "dgp_plan_get_timing: enable timing and run dgp_fit_step first");
  static const int map[TS_COUNT] = {DGP_TIME_GRAM, DGP_TIME_POTRF, DGP_TIME_TRTRI, DGP_TIME_LAUUM, DGP_TIME_SOLVE,
                                    DGP_TIME_GRAD};
  for (int i = 0; i < DGP_TIME_COUNT; ++i) ms_out[i] = 0.0;
  hipError_t e = hipEventSynchronize(p->tev[2 * TS_GRAD + 1]);
  if (e != hipSuccess) return hipfail(e, "hipEventSynchronize");
  for (int st = 0; st < TS_COUNT; ++st) {
    float ms = 0.f;
    e = hipEventElapsedTime(&ms, p->tev[2 * st], p->tev[2 * st + 1]);
    if (e != hipSuccess) return hipfail(e, "hipEventElapsedTime");
    ms_out[map[st]] = ms;
  }
  double sum = 0.0;
  for (int i = 0; i < p->n_syrk; ++i) {
    float ms = 0.f;
    e = hipEventSynchronize(p->sev[2 * i + 1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, p->sev[2 * i], p->sev[2 * i + 1]);
    if (e != hipSuccess) return hipfail(e, "hipEventElapsedTime(syrk)");
    sum += ms;
  }
  ms_out[DGP_TIME_SYRK_SUM] = sum;
  ms_out[DGP_TIME_SYRK_N] = p->n_syrk;
  ms_out[DGP_TIME_SYRK_FLOP] = p->syrk_flop;
  return 0;
}

int dgp_stage_gram(dgp_plan* p, const double* theta, const void* noise, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!theta || !noise) return fail(DGP_E_ARG, "dgp_stage_gram: null argument");
  if (!p->have_inputs) return fail(DGP_E_STATE, "dgp_stage_gram: call dgp_set_inputs first");
  hipStream_t s = (hipStream_t)stream;
  return wrap(DGP_BY_DTYPE(p, run_gram<double>(p, theta, noise, s), run_gram<float>(p, theta, noise, s)), "dgp_stage_gram");
}
int dgp_stage_potrf(dgp_plan* p, void* stream) {
  DGP_CHECK_PLAN(p);
  hipStream_t s = (hipStream_t)stream;
  p->have_inverse = 0;  // S is the factorisation's scratch
  return wrap(DGP_BY_DTYPE(p, run_potrf<double>(p, s), run_potrf<float>(p, s)), "dgp_stage_potrf");
}
int dgp_stage_trtri(dgp_plan* p, void* stream) {
  DGP_CHECK_PLAN(p);
  hipStream_t s = (hipStream_t)stream;
  p->have_inverse = 0;  // S is the inverse's scratch
  return wrap(DGP_BY_DTYPE(p, run_trtri<double>(p, s), run_trtri<float>(p, s)), "dgp_stage_trtri");
}
int dgp_stage_lauum(dgp_plan* p, void* stream) {
  DGP_CHECK_PLAN(p);
  hipStream_t s = (hipStream_t)stream;
  const int rc = DGP_BY_DTYPE(p, run_lauum<double>(p, s), run_lauum<float>(p, s));
  if (!rc) p->have_inverse = 1;
  return wrap(rc, "dgp_stage_lauum");
}
int dgp_stage_solve(dgp_plan* p, const void* r, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!r) return fail(DGP_E_ARG, "dgp_stage_solve: null r");
  hipStream_t s = (hipStream_t)stream;
  int rc = DGP_BY_DTYPE(p, run_solve<double>(p, r, s), run_solve<float>(p, r, s));
  if (!rc) p->have_factor = 1;
  return wrap(rc, "dgp_stage_solve");
}
int dgp_stage_grad(dgp_plan* p, const double* theta, void* dtheta, void* stream) {
  DGP_CHECK_PLAN(p);
  DGP_SINGLE_SITE(p);
  if (!theta || !dtheta) return fail(DGP_E_ARG, "dgp_stage_grad: null argument");
  hipStream_t s = (hipStream_t)stream;
  return wrap(DGP_BY_DTYPE(p, run_grad<double>(p, theta, dtheta, s), run_grad<float>(p, theta, dtheta, s)), "dgp_stage_grad");
}
int dgp_cross_gram(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* Ks, void* stream) {
  DGP_CHECK_PLAN(p);
  DGP_SINGLE_SITE(p);
  if (!theta || !Xs || !work || !Ks || m <= 0) return fail(DGP_E_ARG, "dgp_cross_gram: null argument");
  hipStream_t s = (hipStream_t)stream;
  return wrap(DGP_BY_DTYPE(p, cross<double>(p, theta, Xs, m, work, Ks, s), cross<float>(p, theta, Xs, m, work, Ks, s)),
              "dgp_cross_gram");
}

// The probe runs on the caller-stream's EARLY-INVERSE stream (lowest priority), not on a stream of its own: a process has
// few hardware queues, and one more stream pushes a later single-site plan's rest / bulk streams into a shared queue
// (measured: bench.py's single-site loop 12.1 -> 18.5 ms after a probe on a fresh torch stream).  The load runs on
// `stream` itself (and the library's other internal streams), so the two overlap.
int dgp_debug_clock_probe(void* out_dev, int nwg, double seconds, void* stream) {
  if (!out_dev || nwg < 1 || nwg > 1024 || !(seconds > 0.0) || seconds > 5.0) return fail(DGP_E_ARG, "dgp_debug_clock_probe: bad argument");
  StreamSet* st = stream_set((hipStream_t)stream);
  if (!st) return fail(DGP_E_ARG, "out of host memory");
  const int rc = make_stream(&st->early, false);
  if (rc) return rc;
  clock_probe_kernel<<<dim3((unsigned)nwg), 64, 0, st->early>>>((unsigned long long*)out_dev, (long long)(seconds * 1e8));
  return wrap((int)hipGetLastError(), "dgp_debug_clock_probe");
}

// ---- the leave-one-out predictive likelihood as a training objective (dgp_loo.hip): dgp_fit_step's launches, untouched, into a
// scratch result row, then the passes that read the S and alpha it left.  The plan's A / T / S / z / alpha stay as the step left them.
static LooLayout loo_layout_of(const dgp_plan* p, bool value_only) {
  const Layout L = layout(p);
  return loo_layout(p->N, p->B, value_only ? 0 : p->site_bytes, L.A, L.Tm, L.S, L.alpha, L.gpart);
}
static const char* const LOO_F64 =
    "dgp_loo_*: the leave-one-out objective needs a float64 plan (its bilinear gradient pass exists for float64 only: fp32 plans are "
    "not supported)";

size_t dgp_loo_workspace_bytes(const dgp_plan* p) {
  if (!p || p->dtype != DGP_F64) return 0;
  return loo_layout_of(p, false).total;
}
size_t dgp_loo_value_workspace_bytes(const dgp_plan* p) {
  if (!p || p->dtype != DGP_F64) return 0;
  return loo_layout_of(p, true).total;
}

int dgp_loo_fit_step(dgp_plan* p, const double* theta, const void* r, const void* noise, void* work, size_t work_bytes, void* out,
                     void* dr, void* dnoise, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (p->dtype != DGP_F64) return fail(DGP_E_ARG, LOO_F64);
  DGP_CHECK_PLAN(p);
  if (!theta || !r || !noise || !out) return fail(DGP_E_ARG, "dgp_loo_fit_step: null argument");
  if (!p->have_inputs) return fail(DGP_E_STATE, "dgp_loo_fit_step: call dgp_set_inputs first");
  if (!work || work_bytes < dgp_loo_workspace_bytes(p)) return fail(DGP_E_WORKSPACE, "dgp_loo_fit_step: workspace missing or too small");
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_loo_fit_step: the work area must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const LooLayout L = loo_layout_of(p, false);
  int rc = fit_step<double>(p, theta, r, noise, (char*)work + L.out0, dr, dnoise, 1, s);
  if (rc) return wrap(rc, "dgp_loo_fit_step");
  rc = loo_gradient(p->model, p->d, (const double*)p->Xt, (const double*)p->S, (const double*)p->alpha, p->N, (int)p->n, theta,
                    (const double*)p->dr_w, (char*)work, L, (double*)out, (double*)dr, (double*)dnoise, s, batch_of<double>(p), p->pre);
  return wrap(rc, "dgp_loo_fit_step");
}

int dgp_loo_value(dgp_plan* p, void* work, size_t work_bytes, void* out2, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (p->dtype != DGP_F64) return fail(DGP_E_ARG, LOO_F64);
  DGP_CHECK_PLAN(p);
  if (!out2) return fail(DGP_E_ARG, "dgp_loo_value: null argument");
  if (!p->have_factor || !p->have_inverse)
    return fail(DGP_E_STATE, "dgp_loo_value: needs the K^^-1 a fit step leaves in the plan (dgp_fit_step or dgp_loo_fit_step; dgp_factorize does not form it)");
  if (!work || work_bytes < dgp_loo_value_workspace_bytes(p)) return fail(DGP_E_WORKSPACE, "dgp_loo_value: workspace missing or too small");
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_loo_value: the work area must be 256-byte aligned");
  const int rc = loo_value((const double*)p->S, (const double*)p->alpha, p->info, p->N, (int)p->n, (char*)work, loo_layout_of(p, true),
                           (double*)out2, (hipStream_t)stream, batch_of<double>(p));
  return wrap(rc, "dgp_loo_value");
}

}  // extern "C"
