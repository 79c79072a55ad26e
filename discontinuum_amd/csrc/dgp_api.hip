// dgp_api.hip -- the plan and the fit step: lifecycle, options, batch and site sizes, buffers, timing, the stream sets and the
// stage sequencing of dgp_fit_step / dgp_factorize.  Every other entry point of include/dgp_hip.h lives beside the launchers it
// drives (dgp_predict.hip, dgp_censored.hip, dgp_ep.hip, ...) and reaches the plan through dgp_plan.h.
#include <mutex>
#include <new>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>

#include "dgp_common.h"
#include "dgp_plan.h"

using namespace dgp;

static thread_local char g_err[256] = "";  // the one error text of dgp_last_error() (dgp_plan.h: fail / hipfail / failf)
namespace dgp {
int fail(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}
int hipfail(hipError_t e, const char* where) {
  snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
  return (int)e;
}
int failf(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int factor_ok(dgp_plan* p, hipStream_t s, const char* where) {
  std::vector<int> info((size_t)p->B, 0);
  hipError_t e = hipMemcpy2DAsync(info.data(), sizeof(int), p->info, p->site_bytes, sizeof(int), (size_t)p->B, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hipfail(e, where);
  for (int b = 0; b < p->B; ++b)
    if (info[(size_t)b] != 0) return failf(DGP_E_STATE, "%s: the factorisation the plan holds failed (matrix not positive definite)", where);
  return 0;
}
}  // namespace dgp

enum { TS_GRAM = 0, TS_POTRF, TS_TRTRI, TS_LAUUM, TS_SOLVE, TS_GRAD, TS_COUNT };

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

size_t dgp_plan_workspace_bytes(const dgp_plan* p) { return p ? layout(p).ws_total : 0; }

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
  if (bytes < L.ws_total) return fail(DGP_E_WORKSPACE, "dgp_plan_set_workspace: workspace too small");
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
  p->pre = pre_scratch_bytes(p->B) ? (void*)(p->ws + L.pre) : nullptr;
  p->pre2 = p->pre ? (void*)(p->ws + L.pre2) : nullptr;
  p->nsite = nullptr;
  p->dr_w = nullptr;
  if (p->B > 1) {  // every site starts at the full size n
    p->nsite = (int*)(p->ws + L.nsite);
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

// While the solves run beside lauum on the bulk stream they read the caller's r: a step that leaves early still has to order the
// caller's stream behind them (ev[1]), or the caller may reuse r under the side stream.  Armed once ev[1] is recorded, disarmed
// where the step waits for it itself; nothing is enqueued on the path of a step that succeeds.
struct SolveJoin {
  hipStream_t s;
  hipEvent_t ev;
  bool armed = false;
  ~SolveJoin() {
    if (armed) (void)hipStreamWaitEvent(s, ev, 0);
  }
};

template <typename T>
int dgp::fit_step(dgp_plan* p, const double* theta, const void* r, const void* noise, void* out, void* dr, void* dnoise, int with_grad,
                  hipStream_t s) {
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
  SolveJoin join{s, nullptr};
  if (ov) {
    hipEventRecord(p->ev[1], ss);
    join.ev = p->ev[1];
    join.armed = true;
  }
  p->timed_valid = 0;
  p->have_inverse = 0;
  if (!with_grad && ov) {
    hipStreamWaitEvent(s, p->ev[1], 0);
    join.armed = false;
  }
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
    join.armed = false;
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
template int dgp::fit_step<double>(dgp_plan*, const double*, const void*, const void*, void*, void*, void*, int, hipStream_t);
template int dgp::fit_step<float>(dgp_plan*, const double*, const void*, const void*, void*, void*, void*, int, hipStream_t);

// K(X, X*) for the inference entries of the other units: the test points [B][m][d] to SoA at `work`, the cross Gram to Ks
template <typename T>
int dgp::cross(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* Ks, hipStream_t s, long wbs) {
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
template int dgp::cross<double>(dgp_plan*, const double*, const void*, int64_t, void*, void*, hipStream_t, long);
template int dgp::cross<float>(dgp_plan*, const double*, const void*, int64_t, void*, void*, hipStream_t, long);

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

}  // extern "C"
