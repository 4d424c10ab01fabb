// Host side of the C-ABI (include/blsq.h), shared by its translation units: contexts, the RCCL binding, device buffers,
// the factorisation front end of a plan (QrTree: Gram / certificate / CholeskyQR2 / Householder tree), the CSNE tier's
// host state (CsneTier) and the plan structures.  blsq_ctx.hip: contexts, memory, timing, communicator, diagnostics;
// blsq_front.hip: the bodies of QrTree and CsneTier and the plumbing the step plans' entry points share; blsq_trf.hip: TRF
// and the row-split (TSQR) plans; blsq_dogbox.hip: dogbox plans; blsq_outer.hip: the batched outer drivers and finite differences; blsq_cov.hip: covariance plans; blsq_model.hip: the built-in fit models.
// Internal: nothing here is part of the ABI.
// Ownership: a plan's device memory is freed by its destructor (DevBuf / PinnedBuf, dev_buf.h) — a new buffer is a new
// member and nothing else.  A destroy call synchronises the plan's stream, takes the plan off its ctx and deletes it.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>      // types and prototypes only: the library is dlopen'ed on first use
#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/blsq.h"
#include "blsq_kernels.h"
#include "dev_buf.h"

using namespace blsq;

namespace {

constexpr int RMAX = QR_MAX_TILES * 16;   // rows a workgroup can stage (qr_panel.hip): 1024

enum Slot { K_QR_LEAF = 0, K_QR_MERGE, K_PREP, K_QR_AUG, K_JACOBI, K_STEP, K_LM_GATE, K_LM_QR, K_LM_SOLVE,
            K_GRAM, K_GRAM_CHOL, K_GRAM_GATE, K_AUG_CHOL, K_LM_CHOL, K_CQR2_APPLY, K_CQR2_COMBINE, K_MODEL_EVAL, K_CSNE_PASS,
            K_CSNE_FIX, K_COV_ROWS, K_COV_PINV_WEIGHTS, K_COV_PINV_PRODUCT, K_COV_GATHER, K_COV_INVERSE, K_COV_PRODUCT, K_LOSS_COST, K_LOSS_SCALE, K_NSLOT };
static const char* const kSlotNames[K_NSLOT] = {"qr_leaf", "qr_merge", "prep", "qr_aug", "jacobi_svd", "step",
                                   "lm_gate", "lm_qr", "lm_solve", "gram", "gram_chol", "gram_gate",
                                   "aug_chol", "lm_chol", "cqr2_apply", "cqr2_combine", "model_eval", "csne_pass", "csne_fix",
                                   "cov_rows", "cov_pinv_weights", "cov_pinv_product", "cov_gather", "cov_inverse", "cov_product", "loss_cost", "loss_scale"};

// The ctx's pinned host ints (blsq_ctx::pinned), through which device counters reach the host: 16-byte slots, [0..2] up
// to three counters, [3] the sequence number of a publish (a blocking read leaves it alone).  One slot per use and
// mechanism; a slot is shared only by reads that are consumed before the next one on it starts.
enum PinSlot {
  PIN_OUTER = 0,          // blocking: active / accepted problems of an outer iteration (blsq_outer.hip)
  PIN_GATE,               // blocking: the gate's counters (QrTree::run_gram: 1, the dogbox plans' verdict: 3)
  PIN_GATE_POLLED,        // polled:   the gate's three counters (the TRF plans' verdict)
  PIN_CSNE_LIST,          // blocking: problems left for the tree, problems on the tier (CsneTier::select); relist: the latter
  PIN_CSNE_FAIL,          // blocking: problems the CSNE pass declined (dogbox plans, factor time)
  PIN_CSNE_FAIL_POLLED,   // polled:   the same (TRF plans, step time)
  PIN_LM_ROUND0,          // polled:   active problems of Newton round r in slot PIN_LM_ROUND0 + r, r = 0 .. 12
  PIN_NSLOT = PIN_LM_ROUND0 + 13
};
constexpr int PIN_INTS = 128;             // what blsq_ctx_create allocates
static_assert(4 * PIN_NSLOT <= PIN_INTS, "the last pinned slot ends inside the ctx's pinned ints");

inline int round_up(int v, int q) { return (v + q - 1) / q * q; }
// rows of the stacked systems [R D; E] / [R_aug; sqrt(alpha) I]: two blocks of
// round_up(n, 16) rows each (the second block starts on a tile boundary, see qr_panel.hip)
inline int aug_block_rows(int n) { return (n + 15) / 16 * 16; }
inline int aug_rows(int n) { return 2 * aug_block_rows(n); }

// triangles merged per workgroup: the kernel stages ceil(n/16) tiles of each (>= 2 must fit)
inline int merge_group(int n) { return std::max(2, QR_MAX_TILES / ((n + 15) / 16)); }
inline bool merge_fits(int n) { return 2 * ((n + 15) / 16) <= QR_MAX_TILES; }

}  // namespace


// Device counters -> host without a blit (blsq_ctx.hip; publish_ints, blsq_kernels.h)
__global__ void publish_ints_kernel(const int* __restrict__ src, int n, int* dst, int seq);

static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield" ::: "memory");
#endif
}
struct StepPlan;
struct blsq_ctx {
  blsq_ctx() = default;
  blsq_ctx(const blsq_ctx&) = delete;
  blsq_ctx& operator=(const blsq_ctx&) = delete;
  // (after blsq_ctx_destroy has synchronised the stream; `pinned` and `cq_accept_dev` free themselves)
  ~blsq_ctx() {
    for (auto e : pool) hipEventDestroy(e);
    for (auto e : copy_ev) hipEventDestroy(e);
    if (copy_stream) hipStreamDestroy(copy_stream);
    if (stream) hipStreamDestroy(stream);
  }
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;              // host-pointer API: H2D of the next problems while the Gram of the last runs
  std::vector<hipEvent_t> copy_ev;
  std::string err;
  int timing = 0;                   // 0 off, 1 every slot, 2 + slot: that slot only (blsq_timing_enable)
  bool timing_open = false;         // the last begin() recorded an event
  double t_ms[K_NSLOT] = {0};
  int64_t t_n[K_NSLOT] = {0};
  struct Pending { int slot; hipEvent_t a, b; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> pool;
  PinnedBuf<int> pinned;            // PIN_INTS pinned host ints: device -> host counters without staging (the map:
                                    // PinSlot; touched by pin / read_blocking / read_polled only)
  int pub_seq = 0;                  // sequence number of the last publish()
  blsq::Options opt;                // the switches of this ctx (blsq_options.h: environment at creation, blsq_ctx_set_option)
  long long gram_fast = 0, gram_fallback = 0;   // problems factored by the normal equations / handed to the QR tree
  DevBuf cq_accept_dev;             // device counter (unsigned long long): rejected problems the CholeskyQR2 tier factored
  // CSNE tier (csne_kernels.hip): problems routed to it by factor calls, step-solves it delivered, step-solves it
  // declined (acceptance failed at step time: the problem went on to CholeskyQR2 / the tree)
  unsigned long long csne_routed = 0, csne_steps = 0, csne_declined = 0;
  // collective over the ranks of one tall problem (RCCL over xGMI; blsq_comm_*)
  ncclComm_t comm = nullptr;
  int comm_ranks = 1, comm_rank = 0;
  // plans of this ctx (an optimistic factor call leaves a verdict pending on its plan: blsq_sync and
  // the calls that may invalidate the caller's J resolve it, see ctx_resolve_pending)
  std::vector<StepPlan*> plans;

  int fail(hipError_t e, const char* where) {
    err = std::string(where) + ": " + hipGetErrorString(e);
    return (int)e;
  }
  // n <= 3 device ints -> the 16-byte pinned slot `slot` ([3] = sequence number, returned in *expect)
  hipError_t publish(const int* src, int n, int* slot, int* expect);   // (blsq_ctx.hip)
  // ... and the wait for it: polls the slot; looks at the stream now and then so that a failed launch cannot hang it
  hipError_t await(const int* slot, int expect) {
    for (unsigned long it = 1;; ++it) {
      if (__atomic_load_n(slot + 3, __ATOMIC_ACQUIRE) == expect) return hipSuccess;
      if ((it & 0x3fff) == 0) {
        const hipError_t q = hipStreamQuery(stream);
        if (q == hipSuccess) return __atomic_load_n(slot + 3, __ATOMIC_ACQUIRE) == expect ? hipSuccess : hipErrorUnknown;
        if (q != hipErrorNotReady) return q;
      }
      cpu_relax();
    }
  }
  // The pinned slots (PinSlot).  pin: a slot's address, for a caller that splits publish and await (trf_lm_rounds).
  int* pin(int slot) const { return pinned + 4 * slot; }
  // Blocking read: n <= 3 device ints into the slot by a blit, then the stream is synchronised — it is idle when this
  // returns.  src2 (optional): one more int from elsewhere into [n], by a blit of its own.  *out = the slot.
  hipError_t read_blocking(PinSlot slot, const int* src, int n, const int** out, const int* src2 = nullptr) {
    *out = pin(slot);
    hipError_t e = hipMemcpyAsync(pin(slot), src, n * sizeof(int), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && src2) e = hipMemcpyAsync(pin(slot) + n, src2, sizeof(int), hipMemcpyDeviceToHost, stream);
    return e == hipSuccess ? hipStreamSynchronize(stream) : e;
  }
  // Polled read: publish + await on the slot — no blit, and the stream is not drained.
  hipError_t read_polled(PinSlot slot, const int* src, int n, const int** out) {
    *out = pin(slot);
    int seq = 0;
    const hipError_t e = publish(src, n, pin(slot), &seq);
    return e == hipSuccess ? await(pin(slot), seq) : e;
  }
  int bad(int argidx, const char* what) {
    err = std::string("invalid argument: ") + what;
    return -argidx;
  }
  hipEvent_t get_event() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    // (timing only: without the system-scope fence a default event carries — its cache write-back and invalidation
    //  between every two launches slowed the step it measured by 2-3 %)
    hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
    return e;
  }
  void begin(int slot) {
    timing_open = timing == 1 || (timing >= 2 && timing - 2 == slot);
    if (!timing_open) return;
    Pending p{slot, get_event(), get_event()};
    hipEventRecord(p.a, stream);
    pending.push_back(p);
  }
  void end() {
    if (!timing_open) return;
    timing_open = false;
    hipEventRecord(pending.back().b, stream);
  }
  // The launches of a slot: begin(slot), f() — a callable that launches and returns hipError_t —, end()
  template <class F>
  hipError_t timed(int slot, F&& f) {
    begin(slot);
    const hipError_t e = f();
    end();
    return e;
  }
  // ... and 0, or the failure recorded under `name` (what an entry point returns)
  template <class F>
  int run(int slot, const char* name, F&& f) {
    const hipError_t e = timed(slot, f);
    return e == hipSuccess ? 0 : fail(e, name);
  }
  void collect() {                  // after a stream sync
    for (auto& p : pending) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
        t_ms[p.slot] += ms;
        t_n[p.slot] += 1;
      }
      pool.push_back(p.a);
      pool.push_back(p.b);
    }
    pending.clear();
  }
};
#define HIPCHK(ctx, call)                                   \
  do {                                                      \
    hipError_t e__ = (call);                                \
    if (e__ != hipSuccess) return (ctx)->fail(e__, #call);  \
  } while (0)
namespace blsq_host {

// ---- RCCL, bound at run time ------------------------------------------------------------------
// Only the tall-problem path needs a collective, so librccl (0.5 GB) is not a link-time dependency:
// it is dlopen'ed by the first blsq_comm_* call, from the directory of the HIP runtime this process
// already uses (a host that imported PyTorch first runs on PyTorch's bundled runtime and must get
// the RCCL built against it; everybody else gets /opt/rocm's).
struct Rccl {
  void* lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclGetVersion) GetVersion = nullptr;     // optional
  std::string err, path;
  bool load() {
    if (lib) return true;
    std::vector<std::string> cand;
    Dl_info info;
    // BLSQ_RCCL_PATH: this library and no other (a wrong path is an error, not a reason to look elsewhere)
    const char* forced = getenv("BLSQ_RCCL_PATH");
    if (forced && forced[0]) cand.push_back(forced);
    else if (dladdr((void*)&hipGetDeviceCount, &info) && info.dli_fname) {
      std::string dir(info.dli_fname);
      const size_t k = dir.rfind('/');
      if (k != std::string::npos) {
        dir.resize(k);
        cand.push_back(dir + "/librccl.so.1");
        cand.push_back(dir + "/librccl.so");
      }
    }
    if (!(forced && forced[0])) {
      cand.push_back("librccl.so.1");
      cand.push_back("/opt/rocm/lib/librccl.so.1");
    }
    for (const auto& c : cand) {
      lib = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
      if (lib) { path = c; break; }
    }
    if (!lib) { err = std::string("dlopen(librccl): ") + dlerror(); return false; }
#define BLSQ_RCCL_SYM(name)                                                 \
    name = reinterpret_cast<decltype(name)>(dlsym(lib, "nccl" #name));        \
    if (!name) { err = "librccl lacks nccl" #name; dlclose(lib); lib = nullptr; return false; }
    BLSQ_RCCL_SYM(GetUniqueId) BLSQ_RCCL_SYM(CommInitRank) BLSQ_RCCL_SYM(CommDestroy)
    BLSQ_RCCL_SYM(AllGather) BLSQ_RCCL_SYM(AllReduce) BLSQ_RCCL_SYM(GetErrorString)
#undef BLSQ_RCCL_SYM
    GetVersion = reinterpret_cast<decltype(GetVersion)>(dlsym(lib, "ncclGetVersion"));
    {                                                  // the resolved file, not the name it was asked by
      Dl_info li;
      if (dladdr((void*)GetUniqueId, &li) && li.dli_fname) path = li.dli_fname;
    }
    return true;
  }
};
extern Rccl g_rccl;                             // (blsq_ctx.hip)
constexpr int RCCL_ERR_BASE = 10000;           // return code of a failed RCCL call: 10000 + ncclResult_t

int rccl_fail(blsq_ctx* ctx, ncclResult_t r, const char* where);   // (blsq_ctx.hip)
#define RCCLCHK(ctx, call)                                           \
  do {                                                               \
    ncclResult_t r__ = (call);                                       \
    if (r__ != ncclSuccess) return rccl_fail((ctx), r__, #call);     \
  } while (0)

// One level of the TSQR tree: nleaf workgroups per problem.
struct Level {
  int rowsA, rows_per_leaf, nleaf, RP, LDP;
  DevBuf R;                         // [B][nleaf][NPAD*NPAD]
};

struct QrTree {
  int B = 0, m = 0, n = 0, N = 0, NPAD = 0, NP = 0;
  const blsq::Options* opt = nullptr;      // the ctx's switches (set by build)
  std::vector<Level> levels;        // levels.back().nleaf == 1
  DevBuf V, T;                      // scratch shared by all QR launches of the plan
  // normal-equations fast path (gram_kernels.hip, chol_reg.hip, chol_rl.hip); problems that fail its gate use the levels
  bool gram = false;
  bool want_gram = true;            // false (set before build): Householder tree only, no Gram buffers (covariance plans)
  int gram_nchunk = 1;
  DevBuf gram_part, gram_dsc, gram_ints;   // partial Grams, column scales, [B] fallback mask + count
  DevBuf gram_keep;                 // [B][NPAD*NPAD] the Grams themselves (kept: the trust-region
                                    // systems are diagonal modifications of them)
  DevBuf gram_rinv, gram_ywork, gram_k2;   // conditioning certificate: inverse diagonal tiles, Y = R'^-T, bound [B]
  DevBuf gram_cert;                        // [B] ints: 1 = proven inside the factor kernel (N <= 80)
  DevBuf gram_cflag, gram_ctau;            // [B] certificate stage 3: problems left to the shifted factorisation, their shifts
  double k2_max = 0.0;                     // the gate for this plan's row count (gram_k2_max)
  // CholeskyQR2 middle tier (cqr2_kernels.hip): buffers allocated on first use
  bool cqr2 = false;
  DevBuf cq_W, cq_Wf, cq_G2, cq_R1, cq_R2, cq_z, cq_ints;
  size_t cq_cap = 0;                       // listed problems cq_W / cq_Wf hold (high-water mark of the rejected list)
  bool fb_zeroed = false;                  // the gate counters were cleared by pack_vecs_kernel of this factor call
  // per-problem path of the CURRENT triangles: gram_path()[b] = n + 1 (Householder tree) or 0 (Gram).
  // any_gram / any_qr: whether a problem of either kind can exist (host-side upper bounds)
  bool any_gram = false, any_qr = true;
  bool path_valid = false;          // gram_path() describes the current triangles
  const int* gram_path() const { return gram ? gram_ints.as<int>() + B + 4 : nullptr; }

  // rows: source rows per problem at level 0
  int build(blsq_ctx* ctx, int B_, int rows, int n_, size_t extra_rp_rows);
  // [J f] -> triangle by the normal equations where the conditioning gate allows it.
  // Returns the number of problems left for the Householder tree in *nfallback; their indices
  // are flagged in the fallback mask (n + 1 / 0 per problem).
  // `collective`: the rows of the problem are split over the ranks of ctx->comm — the local Grams
  // are summed over the ranks (ONE ncclAllReduce on the ctx stream) before the factorisation, which
  // is then replicated: every rank holds the same bits, so every rank takes the same gate decision.
  int run_gram(blsq_ctx* ctx, const double* dJ, const double* df, int ldJ, const int* mask,
               int* nfallback, bool collective);
  // Gram front end ONLY: G = [J f]^T [J f] into gram_keep (+ the cross-rank sum); nothing is factored.
  // (k0, nb): problems k0 .. k0 + nb - 1 only (the host-pointer API feeds the Grams in sub-batches behind
  // the copies; the result does not depend on the split — a problem's chunks and their order are functions of m)
  int run_gram_only(blsq_ctx* ctx, const double* dJ, const double* df, int ldJ, const int* mask,
                    bool collective, int k0 = 0, int nb = -1);
  // Householder TSQR tree only (problems selected by ncols_mask; nullptr: all)
  // list / count (optional): compacted indices of the selected problems — a masked launch whose
  // active workgroups alternate with idle ones lands on a fraction of the XCDs
  int run_levels(blsq_ctx* ctx, const double* dJ, const double* df, int ldJ, const int* ncols_mask,
                 const int* list = nullptr, int count = 0);
  // The problems the certificate rejected (fb_list(), nfb of them; fb_mask() = n + 1 for each): a triangle of
  // [J f] of Householder quality into their Rfinal slots — by CholeskyQR2 where its acceptance test passes
  // (second pass over J through the MFMA pipe, cqr2_kernels.hip), by the Householder TSQR tree for the rest.
  int run_fallback(blsq_ctx* ctx, const double* dJ, const double* df, int ldJ, int nfb);
  int* fb_mask() const { return gram_ints.as<int>(); }
  int* fb_count() const { return gram_ints.as<int>() + B; }
  int* path_rw() const { return gram_ints.as<int>() + B + 4; }
  int* fb_list() const { return gram_ints.as<int>() + 2 * (size_t)B + 4; }
  // The tree's share of a plan's factor / certificate arguments (mask: as run): Gram source, gate outputs, certificate
  // scratch and thresholds.  The solver adds its system (G, colscale / diag_vec or ncols_dev / gather), colinfo, pmin_out
  // and its finish block; a launch that wants fewer fields set clears the rest.
  GramCholArgs gate_args(const int* mask) const;
  int run_cert(blsq_ctx* ctx, const GramCholArgs& c);   // the certificate's norm stage + shifted factorisation over c
  // host bookkeeping after a gate verdict: nfb of the problems refreshed by this call failed
  void note_paths(blsq_ctx* ctx, int nfb, bool masked);
  const double* Rfinal() const { return levels.back().R.as<double>(); }

  QrArgs base_args() const {
    QrArgs q{};
    q.opt = opt;
    q.N = N; q.NPAD = NPAD; q.NPmax = NP;
    q.V = V.as<double>(); q.T = T.as<double>();
    return q;
  }
  // [J f] -> R~: by the normal equations where the gate allows it, the Householder tree for the problems it rejects
  // (for all without the Gram front end or f).  ncols_mask (optional, device [B]): problems with an entry <= 1 are
  // skipped — their triangles of the previous run stay in place (outer driver: only fresh Jacobians are factored)
  int run(blsq_ctx* ctx, const double* dJ, const double* df, int ldJ,
          const int* ncols_mask = nullptr, bool collective = false);

 private:
  // the Grams of the `count` problems of g into Gout: launch_gram (several row chunks: partials into Gp), then the
  // reduction of the partials over red_count problems (red_mask) unless the launch has fused it
  hipError_t gram_sum(blsq_ctx* ctx, GramArgs g, double* Gp, double* Gout, int count, const int* red_mask,
                      int red_count);
};

}  // namespace blsq_host
using namespace blsq_host;

// The CSNE tier (csne_kernels.hip), ONE host state for the TRF and the dogbox plans: rejected problems
// whose Gram-Cholesky factor qualifies keep it as a preconditioner, their steps corrected against J in one streaming
// pass.  The select launch and the launches of the correction differ between the solvers and stay with them.
struct CsneTier {
  bool on = false;                  // the plan's shape is supported and option `csne` != 0 (build ran)
  int count = 0;                    // problems on the tier now (host copy of cs.counts[0])
  DevBuf ints;                      // flag [B], list [B], fail_list [B], ne [B], sel_mask [B], counts [4], scratch [4]
  DevBuf pmin, eta, alpha, hp;      // (hp: TRF only)
  DevBuf k2;                        // [B] the bound on kappa_2 of the COMPUTED system (the certificate's own output, gram_k2, keeps its meaning)
  DevBuf vec, part;                 // the recordings (allocated on first use), the partial sums of the pass
  size_t part_cap = 0;              // (list positions x chunks x NE) the partial-sum buffer holds
  CsneState cs{};

  int build(blsq_ctx* ctx, int B, int m, int n, int ld, bool with_hp);   // buffers, zeroed, and cs over them; on = true
  bool ensure_recordings();         // false: no room for them (the caller takes the tier out of service)
  int grow_part(blsq_ctx* ctx, size_t need);
  // the streaming pass over `count` problems: room for its partial sums and a cleared fail counter in front of it; behind
  // it *nfail, read by the caller's mechanism (polled: TRF, blocking: dogbox), into the ctx's statistics
  int pass_begin(blsq_ctx* ctx);
  int pass_verdict(blsq_ctx* ctx, bool polled, int* nfail);
  int relist(blsq_ctx* ctx);        // a masked factor call refreshed some problems: the list from the flags
  int reroute(blsq_ctx* ctx, QrTree& t, int nfail);   // cs.fail_list leaves the tier for t.fb_list()
  // which of the nfb problems the certificate has just rejected (t.fb_list()) the tier takes: the bound from the
  // certificate's norm stage over `chol` (the plan's factor arguments) with CSNE_K2_MAX as its gate, then the plan's
  // select launch; *ntree = the problems left for the other tiers
  int select(blsq_ctx* ctx, QrTree& t, const GramCholArgs& chol, int nfb, int* ntree, bool masked,
             const std::function<hipError_t(const int* sel_mask)>& launch_select);
};

// The optimistic verdict of a device-resident factor call — ONE state machine for the TRF and the dogbox plans
// (verdict_drop / verdict_arm / verdict_resolve below).  blsq_*_factor_dev does not wait for the gate's counters
// (problems that leave the normal-equations path, problems that need the SVD, problems the factor kernel did not
// settle itself): it assumes the common verdict — "none" — and the NEXT call on the plan checks, by which time the
// counters have long arrived.  blsq_*_step_dev enqueues its kernels first and checks afterwards; a wrong guess runs
// the repair (the next tier's factorisation, from the caller's J) and the step once more.
struct VerdictState {
  bool optimistic = true;           // option `optimistic` = 0 switches it off
  bool guess_ok = true;             // the last verdict of this plan was "all fast": only then is the next one guessed
  // Back-off: a plan whose guess keeps failing (inputs that change their conditioning class from call to call) stops
  // guessing for 2, 4, ... 32 factor calls after each wrong guess — a wrong guess costs the Newton rounds and the step
  // once more (about half a step-solve), a synchronous verdict ten microseconds of idle stream; a right guess takes
  // one level off again.
  int guess_streak = 0, guess_pause = 0;
  bool pending = false;
  // Second guess: every problem is settled inside the factor kernel / stage 0 of the certificate, so the certificate
  // and gate launches are not even enqueued; checked with the same read-back.
  bool guess_settled = false, pend_tail = false;
  PinnedBuf<int> pend_pin;          // 4 pinned ints of this plan ([3]: sequence number of the publish)
  int pend_seq = 0;
  bool pend_unpub = false;          // the verdict's counters have not been sent yet: the step kernel of the next
                                    // step call stores them on its way in (or verdict_published() sends them now)
  // the caller's vectors of a device-resident factor call, copied into the state layout by the prep launch
  bool pack_pend = false;
  PackVecs pack_pv{};
  const double* pend_dJ = nullptr; const double* pend_df = nullptr;
  int pend_ldJ = 0, pend_scale_mode = 0;
  double* pend_scale_io = nullptr;
};

// What the TRF and the dogbox plans share: shape, front end, CSNE tier, the staging of the host-pointer API and the
// buffers the shared plumbing reads (step_plan_* / put_state / ... below).
struct StepPlan : VerdictState {
  blsq_ctx* ctx = nullptr;
  int B = 0, m = 0, n = 0, ld = 0;
  QrTree tree;
  // CSNE tier: rejected problems whose steps are corrected against J in one streaming pass (TRF: at step time; dogbox:
  // the Newton step of the free block, at factor time)
  CsneTier csne;
  bool gate_done = false;           // the rank gate already ran in this factor call (no problem left the normal-equations path)
  int njac = -1;                    // problems it sent to the Jacobi SVD (-1: unknown)
  DevBuf vecs;                      // [.][B][ld] n-space vectors; the first four are x, lb, ub, scale in both plans
  DevBuf sweeps, o_scal, o_info;
  DevBuf in_J, in_f, in_scal;       // staging for the host-pointer API
  long long* on_bound = nullptr;    // dogbox: DogState::on_bound
  bool settles_wide = false;        // TRF: stage 0 of the certificate settles problems of N > 80 too (verdict_settled)
  double* vec(int k) const { return vecs.as<double>() + (size_t)k * B * ld; }
  double* scale() const { return vec(3); }
  virtual ~StepPlan() = default;
  virtual int resolve(bool* redo) = 0;   // the verdict of an optimistic factor call (verdict_resolve)
};

struct blsq_trf_plan : StepPlan {
  blsq_trf_plan() { settles_wide = true; }
  // which kernels factor the augmented / Newton systems of the current triangles (per problem:
  // `path`, see trf_after_triangle)
  const int* path = nullptr;
  bool use_chol = false, use_qr = true;
  DevBuf aug_colinfo;               // [B][2] column-norm summary of R_aug (Gram-path problems)
  DevBuf aug_mask;                  // [B] launch mask of the stacked QR of [R D; E] (trf_aug_trivial_kernel)
  DevBuf aug_lam;                   // [B] proven bound on lambda_max of the equilibrated H (LmState::lam)
  DevBuf aug_ym, aug_r1;            // [B] the factor kernel's share of the certificate's stage 0 (GramCholArgs::cert_ym)
  DevBuf aug_open;                  // [B] stage 0's note for the problems it leaves open (GramCholArgs::cert_open)
  DevBuf aug_hmax;                  // [B] largest diagonal entry of H (LmState::hmax: which Newton systems of a
                                    // Householder-path problem may be factored from the Gram)
  bool gram_valid = false;          // tree.gram_keep holds the Grams of the current factor call's problems
  int last_scale_mode = 0;          // scale_mode of the last factor call (a problem that leaves the tier at step time is prepared again)
  // TSQR (multi-rank) extras
  int nranks = 1, m_total = 0;
  bool ranks_agreed = false;        // the ranks have compared their plan configuration (first factor call)
  DevBuf Rcomb;                     // [1][NPAD*NPAD] merged triangle
  DevBuf Rstack;                    // [nranks][NPAD*NPAD] gathered triangles (blsq_tsqr_factor_dev)
  // n-space state
  DevBuf X, scal2;
  DevBuf o_vec, o_hits, o_act;
  TrfState st{};
  TrfStepOut out{};
  double* d_alpha_in = nullptr;
  int aug_RP = 0, aug_LDP = 0;
  // SVD-free trust-region path (lm_kernels.hip)
  DevBuf lm_Xa, lm_ints, lm_sc, lm_ph, lm_sa;
  LmState lm{};
  int lm_enable = 1;                // SVD-free trust-region path allowed at all (BLSQ_NO_SVDFREE)
  int lm_gate_mask = 3;             // launch_lm_gate: bit 0 Householder-path problems, bit 1 normal-equations-path problems
  bool lm_counts_clean = false;     // the Newton-round counters are zero (left so by the last step kernel)
  // The triangle slots st.X hold zeros outside the factors as long as only the Cholesky kernels have
  // written them (zeroed at allocation); the stacked QR and the Jacobi SVD write there.  While clean, the
  // Cholesky of the augmented system does not store those zeros again (half of its bytes).
  bool x_dirty = true;
  int lm_rounds_last = 12;          // Newton rounds that had work in the last step call (run-ahead only over those)
  int resolve(bool* redo) override;      // (blsq_trf.hip)
};

struct blsq_dogbox_plan : StepPlan {
  DevBuf S, X, ivecs, scal2, active, onb;
  DevBuf o_vec, o_onb;
  DevBuf gate_ints;                 // [3B] fast flags, Jacobi launch mask, finished-in-the-Cholesky-kernel flags
  DevBuf colinfo;                   // [B][2] column-norm summary of the free block (Gram-path problems)
  int svdfree_enable = 1;
  DogState st{};
  DogStepOut out{};
  int resolve(bool* redo) override;      // (blsq_dogbox.hip)
};

// ---- shared between the translation units -------------------------------------------------------
namespace blsq_host {
// copy a [B][n] caller vector into the [B][ld] state layout (device to device or host to device, by `kind`)
int put_vec(blsq_ctx* ctx, double* dst, int ld, const double* src, int n, int B, hipMemcpyKind kind);
template <class T>
int get_vec(blsq_ctx* ctx, T* dst, int n, const T* src, int ld, int B) {
  if (!dst) return 0;
  HIPCHK(ctx, hipMemcpy2DAsync(dst, sizeof(T) * n, src, sizeof(T) * ld, sizeof(T) * n, B,
                               hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

// ---- the plumbing the TRF and the dogbox entry points share (blsq_front.hip) ----------------------------------------
// A new plan `p` of either kind, after the entry's own argument checks: the front end (extra_rp_rows: scratch rows beyond
// the tree's own), the plan's alloc_state(), the optimistic verdict's resources (`verdicts`), registration with the ctx.
// On failure p is destroyed.
int step_plan_init(blsq_ctx* ctx, StepPlan* p, int B, int m, int n, size_t extra_rp_rows, bool verdicts,
                   const std::function<int()>& alloc_state);
int step_plan_destroy(StepPlan* p);    // synchronise the stream, take p off its ctx, delete it
// B, m, n and `out` of blsq_{trf,dogbox}_plan_create
int step_plan_args(blsq_ctx* ctx, int B, int m, int n, const void* out);
// J, f, x / lb / ub, scale and scale_mode of the four factor calls
int factor_args(blsq_ctx* ctx, const void* J, const void* f, const void* x, const void* lb, const void* ub,
                const void* scale, int scale_mode);
// staging of a host-pointer factor call: the plan's in_J / in_f (allocated on first use), and J, f into them
int stage_alloc(StepPlan* p);
int stage_upload(StepPlan* p, const double* J, const double* f);
// x, lb, ub, scale (and on_bound: dogbox) of a factor call into the plan's state layout.  Device to device it is one
// pack launch — or, zero_counts in front of a Gram-stage factor call, none: the prep launch of that stage does it
// and clears the gate counters of the call (take_pack)
int put_state(StepPlan* p, const double* x, const double* lb, const double* ub, const double* scale,
              const int64_t* on_bound, hipMemcpyKind kind, bool zero_counts = false);
// the scale a 'jac' scaling mode computed, [B][ld] -> the caller's device [B][n]
int scale_back(StepPlan* p, double* dscale_io, int scale_mode);
// resolve the plan's verdict, copy B items of `item` bytes to the host, blsq_sync
int fetch_resolved(StepPlan* p, void* dst, const void* src, size_t item);
int debug_cond(StepPlan* p, double* k2);   // blsq_{trf,dogbox}_debug_cond
// o_scal / o_info of the last step call on the host, behind everything the entry has enqueued so far (blsq_sync)
int fetch_scal_info(StepPlan* p, std::vector<double>* sc, std::vector<int>* inf);
// The synchronous verdict of a Gram-stage factor call: the gate's three counters by the caller's read mechanism (polled:
// TRF, blocking: dogbox) -> *nfb, gate_done, njac and, after an unmasked call, whether the next call may guess (settles:
// the factor launch counted the problems it did not settle itself, GramCholArgs::unsettled)
int gate_verdict(StepPlan* p, bool polled, bool masked, bool settles, int* nfb);
// the Jacobi SVD of the triangles in X for the problems ncols_dev selects (s, uf, srange: the plan's state vectors)
int run_jacobi(StepPlan* p, double* X, double* s, double* uf, double* srange, const int* ncols_dev);

// Top of a Gram stage: the gate counters fb_count()[0..2] are cleared unless the pack launch does it (fb_zeroed), and
// the deferred vectors of this factor call: handed to the prep launch (returns them), or — a masked call keeps the
// other problems' state, so its prep launch cannot do the copy — packed by the stand-alone launch right here
int take_pack(StepPlan* p, const int* mask, const PackVecs** pk);

// The counters of a pending verdict are on their way to the host (a stand-alone publish unless a step kernel has
// taken them along) — to be called before anything waits for them or overwrites them.
int verdict_published(StepPlan* p);
// blsq_{trf,dogbox}_factor_dev behind their argument checks: the caller's vectors (don_bound: dogbox) into the state
// layout, core() — the plan's factor call, which may leave its verdict pending —, the computed scale back to the caller
template <class Core>
int factor_dev(StepPlan* p, const double* dx, const double* dlb, const double* dub, double* dscale_io, int scale_mode,
               const int64_t* don_bound, Core core) {
  blsq_ctx* ctx = p->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = verdict_published(p);               // (a verdict nobody read: its counters leave before they are cleared)
  if (rc) return rc;
  if ((rc = put_state(p, dx, dlb, dub, dscale_io, don_bound, hipMemcpyDeviceToDevice, true))) return rc;
  p->pend_scale_io = dscale_io;
  if ((rc = core())) return rc;
  return scale_back(p, dscale_io, scale_mode);
}
// ... and the arguments with which the step kernel of this call takes them along (dst == nullptr: nothing to do)
inline PublishArgs verdict_rides(StepPlan* p) {
  if (!p->pend_unpub) return PublishArgs{nullptr, 0, nullptr, 0};
  p->pend_unpub = false;
  p->pend_seq = ++p->ctx->pub_seq;
  return PublishArgs{p->tree.fb_count(), 3, p->pend_pin, p->pend_seq};
}

// the back-off of a plan's guessing (VerdictState::guess_pause)
inline void verdict_wrong(VerdictState* p) {
  if (p->guess_streak < 5) ++p->guess_streak;
  p->guess_pause = 1 << p->guess_streak;
}
inline void verdict_right(VerdictState* p) { if (p->guess_streak > 0) --p->guess_streak; }
// may this factor call guess?  (consumes one call of a pause)
inline bool verdict_may_guess(VerdictState* p) {
  if (p->guess_pause > 0) { --p->guess_pause; return false; }
  return p->optimistic && p->guess_ok;
}

// has the factor kernel (N <= 80) / stage 0 of the certificate (TRF, N > 80) settled every problem of the call?
inline bool verdict_settled(const StepPlan* p) { return (p->settles_wide || p->ld <= 80) && p->pend_pin[2] == 0; }

// A verdict nobody asked for belongs to a factor that is being overwritten (top of a factor call): no repair, but it is
// still read — the path statistics and the decision whether to guess again depend on it.
int verdict_drop(StepPlan* p);

// The counters of this factor call ride on the next step kernel (verdict_rides; verdict_published sends them if nothing
// took them along); the verdict is read by verdict_resolve.  skip_tail: the second guess — the gate launches were not
// enqueued.
inline void verdict_arm(StepPlan* p, bool skip_tail, const double* dJ, const double* df, int ldJ, int scale_mode) {
  p->pend_unpub = true;
  p->pending = true; p->pend_tail = skip_tail;
  p->pend_dJ = dJ; p->pend_df = df; p->pend_ldJ = ldJ; p->pend_scale_mode = scale_mode;
  p->gate_done = true;
  p->njac = 0;
}

// The verdict of an optimistic factor call.  *redo = false: nothing was pending, or the guess held.  *redo = true: it
// did not — after `repair` the state is what the synchronous path would have left, and whatever was computed from the
// guessed state must be computed again.  gate_tail(): the launches the second guess left out (certificate, rank gate);
// repair(nfb): the plan's own way from "nfb problems left the normal-equations path" to a finished factor state.
template <class GateTail, class Repair>
int verdict_resolve(StepPlan* p, bool* redo, GateTail gate_tail, Repair repair) {
  if (redo) *redo = false;
  if (!p->pending) return 0;
  blsq_ctx* ctx = p->ctx;
  QrTree& t = p->tree;
  p->pending = false;
  { int rc_ = verdict_published(p); if (rc_) return rc_; }
  HIPCHK(ctx, ctx->await(p->pend_pin, p->pend_seq));
  int nfb = p->pend_pin[0], njac = p->pend_pin[1];
  const bool settled = verdict_settled(p);
  if (p->pend_tail) {
    if (settled) return 0;                  // (settled: certified and finished in the factor kernel — nfb = njac = 0)
    // wrong second guess: the launches that were left out, then the verdict as a synchronous call reads it
    p->guess_settled = false;
    if (redo) *redo = true;
    { int rc_ = gate_tail(); if (rc_) return rc_; }
    HIPCHK(ctx, hipMemcpyAsync(p->pend_pin, t.fb_count(), 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    nfb = p->pend_pin[0]; njac = p->pend_pin[1];
    if (nfb > 0 || njac > 0) { p->guess_ok = false; verdict_wrong(p); }
  } else {
    p->guess_settled = settled;
    if (nfb == 0 && njac == 0) { verdict_right(p); return 0; }
    p->guess_ok = false;
    verdict_wrong(p);
    if (redo) *redo = true;
  }
  ctx->gram_fast -= nfb; ctx->gram_fallback += nfb;      // (note_paths counted everybody as fast)
  t.any_qr = nfb > 0; t.any_gram = nfb < p->B; t.path_valid = true;
  p->gate_done = (nfb == 0);
  p->njac = p->gate_done ? njac : -1;
  { int rc_ = repair(nfb); if (rc_) return rc_; }
  return scale_back(p, p->pend_scale_io, p->pend_scale_mode);
}

// the whole factor call of a plan from device-resident [J f] (mask: outer driver, fresh Jacobians only)
// (blsq_trf.hip / blsq_dogbox.hip)
int trf_factor_core(blsq_trf_plan* p, const double* dJ, const double* df, int ldJ, int scale_mode,
                    const int* mask, bool may_defer = false, bool gram_done = false);
int dog_factor_core(blsq_dogbox_plan* p, const double* dJ, const double* df, int ldJ, int scale_mode,
                    const int* mask, bool may_defer = false);
// every verdict an optimistic factor call left pending on a plan of this ctx is read, and a wrong guess repaired
int ctx_resolve_pending(blsq_ctx* ctx);
}  // namespace blsq_host

// Covariance plan (blsq_cov.hip): the Householder tree of a plain J and the n-space tail of cov_kernels.hip
struct blsq_cov_plan {
  blsq_ctx* ctx = nullptr;
  int B = 0, m = 0, n = 0;
  QrTree tree;                      // want_gram = false: run_levels only
  // m > 1024 with n > 512 is past the tree's merge capacity: such a plan folds the rows in sequentially instead —
  // the first 1024 rows, then [R; next rows] as a dense leaf of at most 1024 rows, until J is used up
  bool fold = false;
  int NPAD = 0;                     // leading dimension of the triangles (tree.NPAD, or the fold's)
  DevBuf fR, fS, fV, fT;            // fold: triangles [B][NPAD*NPAD], stack [B][1024][NPAD], reflector scratch
  const double* Rfinal() const { return fold ? fR.as<double>() : tree.Rfinal(); }
  DevBuf zf;                        // [B][m] zeros: the right-hand side column the tree carries along
  DevBuf X;                         // [B][NPAD*NPAD] the explicit inverse
  DevBuf perm, nfree, Jp;           // 'free' mode, allocated on first use: permutation, free counts, gathered J
  DevBuf in_J, in_act, o_cov, o_rcond, o_status;   // staging of the host-pointer call, allocated on first use
  // pseudo-inverse route (blsq_cov_pinv*), allocated on first use: the Jacobi kernel's s, uf [B][NPAD], srange [B][2],
  // sweeps [B], per-problem widths nfree + 1 [B]; the weights [B][NPAD]; staging of the host-pointer call
  DevBuf js, juf, jsrange, jsweeps, jncols, pw;
  DevBuf in_scale, o_rank, o_kept;
  // What the last covariance call left behind for blsq_cov_rows* (DESIGN.md 7i): the route — the regular one keeps
  // X = R^-1 in its slot, the pinv one the rotated triangle and pw —, whether perm / nfree describe it, whether in_J
  // still holds the J of a host-pointer call, and the plan's own copy of the per-problem status
  enum Kept { KEPT_NONE = 0, KEPT_REGULAR, KEPT_PINV };
  Kept kept = KEPT_NONE;
  bool kept_masked = false, kept_staged = false;
  bool kept_refined = false;        // pinv route: the X slot holds the refined factor of this covariance call
  DevBuf kept_status;               // [B]
  DevBuf rowgram;                   // pinv route, allocated on first use: [B][NPAD*NPAD] W W^T (launch_cov_pinv_rowfactor)
  DevBuf r_A, r_scale, r_out;       // staging of the host-pointer rows call, grown on demand: [B][rows][n], [B], [B][rows]
};
namespace blsq_host {
// the whole covariance call on device pointers; dactive: int64 [B][lda] or nullptr
int cov_core(blsq_cov_plan* p, const double* dJ, const long long* dactive, int lda, double* dcov, double* drcond,
             int* dstatus);
// ... and with host outputs through the plan's own device buffers (blsq_outer_covariance)
int cov_to_host(blsq_cov_plan* p, const double* dJ, const long long* dmask, int lda, double* cov, double* rcond,
                int32_t* status);
// the pseudo-inverse route on device pointers (dscale [B] or nullptr), and with host outputs (blsq_outer_covariance_pinv)
int cov_pinv_core(blsq_cov_plan* p, const double* dJ, const long long* dactive, int lda, const double* dscale,
                  double* dcov, int* drank, double* drcond, double* dkept, int* dstatus);
int cov_pinv_to_host(blsq_cov_plan* p, const double* dJ, const long long* dmask, int lda, const double* dscale,
                     double* cov, int32_t* rank, double* rcond, double* kept_rcond, int32_t* status);
// out[b][i] = scale[b] |a_i through the kept factor|^2 for the rows of dA [B][rows][n] (blsq_cov_rows_dev without its
// argument checks; blsq_outer_leverage)
int cov_rows_core(blsq_cov_plan* p, int rows, const double* dA, const double* dscale, double* dout);
}  // namespace blsq_host

