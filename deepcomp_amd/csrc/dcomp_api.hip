// dcomp_api.hip -- C ABI (include/dcomp.h) of libdcomp_hip.so: handle management, kernel dispatch,
// the CPython-compatible Mersenne-Twister tape generator, device self-tests.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#define DCOMP_BUILDING_LIBRARY 1     // (no dcomp_create -> dcomp_create_v macro in here)
#include "../../include/dcomp.h"
#include "dcomp_blist.h"
#include "dcomp_device.h"
#include "dcomp_fragment.h"
#include "dcomp_big.h"

namespace dcomp {
#define DCOMP_DECL(n) KernelPair kernels_b##n(int upad, int mp);
DCOMP_B_LIST(DCOMP_DECL)
#undef DCOMP_DECL

static KernelPair lookup_kernels(int B, int upad, int mp)
{
    switch (B) {
#define DCOMP_CASE(n) case n: return kernels_b##n(upad, mp);
        DCOMP_B_LIST(DCOMP_CASE)
#undef DCOMP_CASE
    default: return KernelPair{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    }
}
}  // namespace dcomp

using dcomp::KParams;
using dcomp::UeCfg;

static thread_local char g_err[512] = "";
static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
// the other objects of the library (dcomp_actor.hip) report through the same thread-local text
namespace dcomp { int report(int code, const char *msg) { return fail(code, "%s", msg); } }
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(DCOMP_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// Environment overrides (tests and A/B runs), read ONCE per handle by dcomp_create_v: INTEGRATION.md section 2 has the table of
// names, values, effects and users.
struct EnvInt { bool set; long v; };
struct Overrides { EnvInt force_big, no_fused_big, dsq_exact, big_row_x4, wide_pad_lds, fuse_max_waves, tight, fused_row_limit_log2; };
static Overrides read_overrides()
{
    auto get = [](const char *name) { const char *e = getenv(name); return EnvInt{e != nullptr, e ? atol(e) : 0}; };
    return Overrides{get("DCOMP_FORCE_BIG"), get("DCOMP_NO_FUSED_BIG"), get("DCOMP_DSQ_EXACT"), get("DCOMP_BIG_ROW_X4"),
                     get("DCOMP_WIDE_PAD_LDS"), get("DCOMP_FUSE_MAX_WAVES"), get("DCOMP_TIGHT"), get("DCOMP_FUSED_ROW_LIMIT_LOG2")};
}

// The launch plan of a handle: which kernels it launches and how, decided once by make_plan (dcomp_create_v) and only read afterwards.
// StepPath, the step kernel: Special = step_kernel (padded power-of-two lane groups), Wide = step_kernel_wide (one workgroup per env slot),
// Dyn = step_kernel_dyn (the UE list changes: cfg.max_ues > 0), Tight = step_kernel_tight (U lanes per env), Generic = big_kernel
// (dcomp_big.h: 33 ... 64 stations, more than DCOMP_SPECIAL_MAX_UE slots, or DCOMP_FORCE_BIG=1).
// Fuse, what dcomp_rollout does with T steps: None = the step kernel once per step, Always = one launch of the fused rollout kernel,
// Long = that for rollouts of >= 4 steps and for the closed loop only, Stretch = the generic kernel's: one launch per stretch of an episode.
enum class StepPath { Special, Wide, Dyn, Tight, Generic };
enum class Fuse { None, Always, Long, Stretch };
enum class Launch { Reset, Step, Rollout };
struct LaunchPlan {
    StepPath path = StepPath::Special;
    Fuse fuse = Fuse::None;
    // the specialised kernels (path != Generic); rollout / rollout_pol: the fused rollout without / with the in-step policy
    dcomp::KernelFn reset = nullptr, step = nullptr, rollout = nullptr, rollout_pol = nullptr;
    bool tight_central = false;        // Tight: `step` is the central-only instantiation (dcomp_step_kernel_name)
    bool rollout_tight = false;        // `rollout` is the tightly packed instantiation: launched with the tight grid and packing
    dcomp::BigKernels big{};           // the generic kernel (path == Generic)
    int big_step = 0;                  // BigKernels::fn's `which` of a step: 0, or 2 with UE arrival / departure
    int grid = 0, block = DCOMP_BLOCK;
    size_t lds = 0;                    // dynamic LDS per workgroup: Generic every launch (big_carve); Wide the steps that write rows (occupancy cap)
    int lanes = 0;                     // lanes per env: the padded width, or U when the step is tightly packed
    int tight_grid = 0, tight_g = 0, tight_gpw = 0, tight_magic = 0;   // the tight packing (KParams::tight_*), 0 = off
    uint64_t row_limit = 0;            // rows (num_steps * num_envs * num_ue) from which an every-step fragment no longer fits the fused rollout kernel
};
struct dcomp_env {
    dcomp_cfg cfg;
    KParams kp;                 // constant part pre-filled
    Overrides ovr;
    LaunchPlan plan;            // decided by dcomp_create_v, read-only afterwards
    UeCfg *d_ue_cfg = nullptr;
    double2 *d_ue_velq = nullptr;   // {velocity, qmax} of UEs whose fixed velocity is no integer in 0..255 (cfg.ue_velocity)
    bool dyn;                  // UE list changes during an episode (cfg.max_ues > 0)
    int mp_pattern;            // sharing-pattern specialisation the kernels were looked up with (dcomp::MP_*)
    int upad;                  // padded lanes per env
    int cap, cur_ue;            // slots per env; UEs currently listed
    uint32_t n_removed = 0, n_arrived = 0;   // this episode (Philox draw words)
    int time = 0;
    int64_t episode = -1;       // index of the current episode (-1 before the first reset)
    dcomp::BigParams bigp{};   // the generic kernel's second argument
    double2 *d_bs = nullptr;
    int32_t *d_mode = nullptr;
};
struct EnvDeleter { void operator()(dcomp_env *env) const { dcomp_destroy(env); } };

// ---- channel constants from the reference's own formula (station.py:26-30,110-127), FP64 on the host ----
struct PathLoss { double c1, c2; };     // pl(d) = c1 + c2 * log10(d)
static PathLoss path_loss()
{
    const double f = 2500.0, hb = 50.0, hu = 1.5;
    const double ch = 0.8 + (1.1 * std::log10(f) - 0.7) * hu - 1.56 * std::log10(f);
    return PathLoss{69.55 + 26.16 * std::log10(f) - 13.82 * std::log10(hb) - ch, 44.9 - 6.55 * std::log10(hb)};
}
static double ref_snr(double d)
{
    const double tx = 30.0, noise = 1e-9;
    const PathLoss c = path_loss();
    double pl = c.c1 + c.c2 * std::log10(d + 1e-16);
    return std::pow(10.0, (tx - pl) / 10.0) / noise;
}
// d_T = the smallest double d whose snr, computed the reference's way, is NOT above the threshold; -1 when that computed snr is not
// monotone within 4 096 doubles either side of d_T (then `d < d_T` would not be the reference's decision; dcomp_create refuses).
static double connect_threshold_checked()
{
    static const double cached = [] {
        double lo = 60.0, hi = 80.0;    // snr(lo) > 2e-8 >= snr(hi)
        for (int i = 0; i < 200; i++) {
            double mid = 0.5 * (lo + hi);
            if (mid == lo || mid == hi) break;
            if (ref_snr(mid) > 2e-8) lo = mid; else hi = mid;
        }
        double below = hi, above = hi;
        for (int k = 0; k < 4096; k++) {
            below = std::nextafter(below, 0.0);
            if (!(ref_snr(below) > 2e-8) || ref_snr(above) > 2e-8) return -1.0;
            above = std::nextafter(above, INFINITY);
        }
        return hi;
    }();
    return cached;
}
extern "C" double dcomp_connect_threshold(void) { return connect_threshold_checked(); }
// The reference decides `snr(sqrt(dx*dx + dy*dy)) > 2e-8` (station.py:122-127, 222-226): with q = fl(fl(dx*dx) + fl(dy*dy)) -- two rounded
// squares, one rounded sum, contraction off -- that is sqrt_rn(q) < d_T, and since the correctly rounded root is monotone,
//     in range  <=>  q < X,   X = the smallest double q with sqrt_rn(q) >= d_T.
// X is NOT fl(d_T * d_T) (one ulp above X for the reference's constants): the kernels compare against X (KParams::dt2), found here by
// walking the doubles around d_T * d_T with the host's IEEE sqrt (checked against brute force in dcomp_create, qmax(v)).
extern "C" double dcomp_connect_boundary_sq(void)
{
    const double dt = connect_threshold_checked();
    if (!(dt > 0.0)) return -1.0;
    double q = dt * dt;
    while (std::sqrt(q) >= dt) q = std::nextafter(q, 0.0);
    while (std::sqrt(q) < dt) q = std::nextafter(q, INFINITY);
    return q;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the FUNCTION on a DEVICE, shared by every env that launches it: it only ever
// goes UP -- a running maximum per (function, device) -- so that a later env with a smaller footprint does not lower the limit under an
// earlier one.  (Asking for the CU's whole 160 KB once and for all is refused by the runtime: "invalid argument".)
static hipError_t raise_lds_limit(const void *fn, int bytes)
{
    struct Raised { const void *fn; int dev, bytes; };
    static std::mutex mu;
    static std::vector<Raised> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    for (auto &d : done) {
        if (d.fn != fn || d.dev != dev) continue;
        if (d.bytes >= bytes) return hipSuccess;
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess) d.bytes = bytes;
        return e;
    }
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.push_back(Raised{fn, dev, bytes});
    return e;
}

static int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// Floats per observation row of one UE (variants.py: multi-agent connected | dr | ues_at_bs | util_at_bs | utility, central connected | dr | utility).
static int row_floats(int env_kind, int B) { return env_kind == DCOMP_MULTI ? 4 * B + 1 : 2 * B + 1; }

extern "C" const char *dcomp_last_error(void) { return g_err; }
#define DCOMP_STR2(x) #x
#define DCOMP_STR(x) DCOMP_STR2(x)
extern "C" const char *dcomp_version(void) { return "deepcomp_amd 0.2 (gfx950, ABI " DCOMP_STR(DCOMP_ABI_VERSION) ")"; }
extern "C" int dcomp_abi_version(void) { return DCOMP_ABI_VERSION; }

// The version-1 entry point.  A binary that still calls it was compiled against structs this library no longer reads the same way
// (dcomp_out had six pointers): refuse instead of reading past them.
extern "C" int dcomp_create(const dcomp_cfg *, dcomp_env **out)
{
    if (out) *out = nullptr;
    return fail(DCOMP_EABI, "dcomp_create is the ABI-1 entry point and this library is ABI %d: rebuild the caller against include/dcomp.h "
                            "(its dcomp_create macro calls dcomp_create_v) or call dcomp_create_v with the caller's struct sizes", DCOMP_ABI_VERSION);
}

// ---- dcomp_create_v in steps: validate, per-UE tables, channel constants, launch plan, device uploads ----
// What can be wrong with a configuration -- the velocities and utilities: ue_tables -- before anything is allocated.
static int validate_cfg(const dcomp_cfg *cfg)
{
    const int E = cfg->num_envs, U = cfg->num_ue, B = cfg->num_bs;
    if (E < 1 || U < 1 || U > DCOMP_MAX_UE || B < 1 || B > DCOMP_MAX_BS)
        return fail(DCOMP_EINVAL, "need num_envs>=1, 1<=num_ue<=%d, 1<=num_bs<=%d (got %d, %d, %d)", DCOMP_MAX_UE, DCOMP_MAX_BS, E, U, B);
    const int CAP = cfg->max_ues > 0 ? cfg->max_ues : U;           // slots per env (base.py:79-84)
    if (CAP < U) return fail(DCOMP_EINVAL, "max_ues (%d) < num_ue (%d)", CAP, U);                 // base.py:84
    if ((int64_t)E * CAP > (int64_t)1 << 30) return fail(DCOMP_EINVAL, "num_envs*max_ues too large");
    if (cfg->map_w < 3 || cfg->map_h < 3 || cfg->map_w > 65535 || cfg->map_h > 65535)
        return fail(DCOMP_EINVAL, "map must be 3..65535 in both dimensions");
    for (int u = 0; u < U; u++) {                                  // RandomWaypoint(pause_duration, border_buffer), movement.py:87-104
        const int pd = cfg->ue_pause_duration ? cfg->ue_pause_duration[u] : 2, bb = cfg->ue_border_buffer ? cfg->ue_border_buffer[u] : 10;
        if (pd < 0 || pd > 127) return fail(DCOMP_EINVAL, "ue %d: pause_duration %d outside 0..127 (7 bits of the movement word)", u, pd);
        if (bb < 1 || bb > 255) return fail(DCOMP_EINVAL, "ue %d: border_buffer %d outside 1..255 (movement.py:103 asserts > 0)", u, bb);
        if (cfg->map_w < 2 * bb + 1 || cfg->map_h < 2 * bb + 1)
            return fail(DCOMP_EINVAL, "ue %d: map %dx%d leaves no waypoint inside a border buffer of %d", u, cfg->map_w, cfg->map_h, bb);
    }
    if (cfg->max_ues > 0 && (cfg->map_w < 21 || cfg->map_h < 21))
        return fail(DCOMP_EINVAL, "UE arrival needs a map of at least 21x21 (arriving UEs use border_buffer 10, base.py:597-599)");
    if (cfg->env_kind != DCOMP_CENTRAL && cfg->env_kind != DCOMP_MULTI) return fail(DCOMP_EINVAL, "bad env_kind");
    if (cfg->reward_agg < 0 || cfg->reward_agg > 2) return fail(DCOMP_EINVAL, "bad reward_agg");
    if (cfg->rng_mode != DCOMP_RNG_TAPE && cfg->rng_mode != DCOMP_RNG_PHILOX) return fail(DCOMP_EINVAL, "bad rng_mode");
    if (cfg->rng_mode == DCOMP_RNG_TAPE && cfg->tape_depth < 1) return fail(DCOMP_EINVAL, "tape mode needs tape_depth >= 1");
    if (!cfg->bs_x || !cfg->bs_y || !cfg->bs_sharing || !cfg->ue_vel_lo || !cfg->ue_vel_hi)
        return fail(DCOMP_EINVAL, "bs_x, bs_y, bs_sharing, ue_vel_lo, ue_vel_hi are required");
    for (int b = 0; b < B; b++)
        if (cfg->bs_sharing[b] < 0 || cfg->bs_sharing[b] > 3) return fail(DCOMP_EINVAL, "bs_sharing[%d]=%d not supported", b, cfg->bs_sharing[b]);   // station.py:22
    return DCOMP_OK;
}

// KParams' constant part: shape, seeds, the channel constants, the station table.  Refuses a host whose libm / sqrt would not
// reproduce the reference's range decision or the kernels' closed form of qmax.
static int fill_constants(dcomp_env *env, const dcomp_cfg *cfg, const std::vector<UeCfg> &uc)
{
    const int U = cfg->num_ue, B = cfg->num_bs;
    KParams &kp = env->kp;
    std::memset(&kp, 0, sizeof(kp));
    kp.E = cfg->num_envs; kp.U = env->cap; kp.U0 = U; kp.cur_ue = U; kp.tape_ids = U;
    kp.map_w = cfg->map_w; kp.map_h = cfg->map_h;
    kp.kind = cfg->env_kind; kp.reward_agg = cfg->reward_agg; kp.rng_mode = cfg->rng_mode;
    kp.tape_depth = cfg->tape_depth;
    kp.seed_lo = (uint32_t)cfg->seed; kp.seed_hi = (uint32_t)(cfg->seed >> 32);
    kp.env_base = (uint32_t)cfg->env_id_base;
    // snr = K * (d + eps)^(-gamma): gamma = c2/10, K = snr(1 m)   (station.py:110-127); c1 / c2 also feed the kernel's FP64 max-cap rate key
    const PathLoss pl = path_loss();
    kp.pl_c1 = pl.c1; kp.pl_c2 = pl.c2;
    kp.half_gamma = (float)(pl.c2 / 20.0);
    kp.log2k = (float)(std::log2(ref_snr(1.0)) + (double)dcomp::L2_OFF);
    kp.log2k_s = (float)(std::log2(ref_snr(1.0)) + (double)dcomp::L2_OFF - 12.0 * (pl.c2 / 20.0));
    kp.dt2 = dcomp_connect_boundary_sq();       // X: q < X  <=>  snr(sqrt(q)) > 2e-8 in the reference's own arithmetic
    if (!(kp.dt2 > 0.0)) return fail(DCOMP_EUNSUPPORTED, "the host's log10 / pow make snr(d) non-monotone around the connect threshold: d < d_T would not be the reference's decision");
    // the kernels decide on a FUSED d^2 and redo a pair in the reference's form when (float)fused == (float)X (dcomp_device.h, dist_sq_ref):
    // sound iff every double within 4 ulp of X has the float image of X -- else every pair takes the reference form
    kp.dt2f = (float)kp.dt2;
    double lo = kp.dt2, hi = kp.dt2;
    for (int k = 0; k < 4; k++) { lo = std::nextafter(lo, 0.0); hi = std::nextafter(hi, INFINITY); }
    kp.dsq_exact = ((float)lo == kp.dt2f && (float)hi == kp.dt2f) ? 0u : 1u;
    if (env->ovr.dsq_exact.set && env->ovr.dsq_exact.v != 0) kp.dsq_exact = 1u;      // tests: the always-exact path
    for (unsigned v = 0; v < 256; v++) {
        // the kernel's closed form of qmax(v) = max{q : sqrt_rn(q) <= v} (move_ue) against brute force
        double q = (double)(v * v);
        while (std::sqrt(std::nextafter(q, INFINITY)) <= (double)v) q = std::nextafter(q, INFINITY);
        double cf = (double)(v * v);
        if (v > 0) {
            int e2 = 2 * (31 - __builtin_clz(v));
            if (v * v < (2u << e2)) cf += std::ldexp(1.0, e2 - 52);
        }
        if (cf != q) return fail(DCOMP_EUNSUPPORTED, "host sqrt is not IEEE-correct: qmax(%u) mismatch", v);
    }
    for (int b = 0; b < B; b++) {
        const int m = cfg->bs_sharing[b];
        if (b < DCOMP_MASK32_MAX_BS) { kp.bs_x[b] = cfg->bs_x[b]; kp.bs_y[b] = cfg->bs_y[b]; kp.bs_mode[b] = m; }
        if (m == DCOMP_MAX_CAP) { kp.any_maxcap = 1; if (b < 32) kp.maxcap_mask |= 1u << b; env->bigp.maxcap_mask |= 1ull << b; }
        if (m == DCOMP_RATE_FAIR || m == DCOMP_PROP_FAIR) { kp.any_sum_mode = 1; env->bigp.summode_mask |= 1ull << b; }
    }
    env->bigp.B = B;
    kp.all_log_util = 1;
    for (const UeCfg &c : uc) if (c.util != DCOMP_UTIL_LOG) kp.all_log_util = 0;
    return DCOMP_OK;
}

// The per-UE tables the kernels read from device memory, checked entry by entry while they are built (on the host).  uc: the UE's
// configuration.  vq: {v, qmax(v)} of UEs whose fixed velocity is no integer in 0..255 (movement.py:116-117 / 142-156), qmax(v) = largest
// double q with sqrt_rn(q) <= v -- `distance <= velocity` without a square root, as for the integers; empty when there is no such UE.
static int ue_tables(const dcomp_cfg *cfg, std::vector<UeCfg> &uc, std::vector<double> &vq)
{
    for (int u = 0; u < cfg->num_ue; u++) {
        const int lo = cfg->ue_vel_lo[u], hi = cfg->ue_vel_hi[u];
        if (lo < 0 || hi < lo || hi > 255) return fail(DCOMP_EINVAL, "ue %d: velocity range [%d,%d] invalid", u, lo, hi);
        UeCfg c;
        std::memset(&c, 0, sizeof(c));
        c.vel_lo = (uint8_t)lo; c.vel_hi = (uint8_t)hi;
        c.init_x = cfg->ue_init_x ? (int16_t)cfg->ue_init_x[u] : (int16_t)-1;
        c.init_y = cfg->ue_init_y ? (int16_t)cfg->ue_init_y[u] : (int16_t)-1;
        c.util = cfg->ue_util ? (uint8_t)cfg->ue_util[u] : (uint8_t)DCOMP_UTIL_LOG;
        if (c.util > DCOMP_UTIL_STEP) return fail(DCOMP_EUNSUPPORTED, "ue %d: utility %d not implemented", u, (int)c.util);   // user.py:92
        c.dr_req = cfg->ue_dr_req ? cfg->ue_dr_req[u] : 1.0f;
        c.pause = (uint8_t)(cfg->ue_pause_duration ? cfg->ue_pause_duration[u] : 2);
        c.border = (uint8_t)(cfg->ue_border_buffer ? cfg->ue_border_buffer[u] : 10);
        uc.push_back(c);
        const double v = cfg->ue_velocity ? cfg->ue_velocity[u] : -1.0;
        if (!(v >= 0.0)) continue;
        if (!std::isfinite(v) || v > 1e6) return fail(DCOMP_EINVAL, "ue %d: velocity %g out of range", u, v);
        if (lo != hi) return fail(DCOMP_EINVAL, "ue %d: ue_velocity needs a fixed range (lo == hi)", u);
        double q = v * v;
        while (q > 0.0 && std::sqrt(q) > v) q = std::nextafter(q, 0.0);
        while (std::sqrt(std::nextafter(q, INFINITY)) <= v) q = std::nextafter(q, INFINITY);
        if (vq.empty()) vq.assign(2 * (size_t)cfg->num_ue, -1.0);
        vq[2 * u] = v; vq[2 * u + 1] = q;
    }
    return DCOMP_OK;
}

// Which kernels this handle launches, with which grid, block and LDS -- the only place that decides it (needs kp.any_maxcap).
static int make_plan(dcomp_env *env)
{
    const dcomp_cfg &cfg = env->cfg;
    const Overrides &ovr = env->ovr;
    LaunchPlan &pl = env->plan;
    const int E = cfg.num_envs, B = cfg.num_bs, CAP = env->cap;
    const bool DYN = env->dyn, central = cfg.env_kind == DCOMP_CENTRAL;
    const double row_bytes = (double)E * CAP * row_floats(cfg.env_kind, B) * 4.0;     // one step's observation rows
    pl.lanes = env->upad;
    const long l2 = ovr.fused_row_limit_log2.v;                    // (tests: the one-launch-per-step fallback without a 2^31-row fragment)
    pl.row_limit = (uint64_t)1 << (ovr.fused_row_limit_log2.set && l2 >= 1 && l2 <= 31 ? l2 : 31);
    // More than 32 stations: the generic kernel (dcomp_big.h; one instantiation per lane width, B a run-time value, connection set in two
    // state words).  DCOMP_FORCE_BIG=1 sends smaller station counts there too (tests: generic against specialised kernels).
    if (B > DCOMP_MASK32_MAX_BS || CAP > DCOMP_SPECIAL_MAX_UE || (ovr.force_big.set && ovr.force_big.v != 0)) {
        pl.path = StepPath::Generic;
        pl.big = dcomp::big_kernels_for_upad(env->upad);
        if (!pl.big.fn[0][0][0]) return fail(DCOMP_EUNSUPPORTED, "no generic kernel for %d lanes per env", env->upad);
        pl.big_step = DYN ? 2 : 0;
        if (!DYN && !ovr.no_fused_big.set) pl.fuse = Fuse::Stretch;   // (the fused rollout steps a fixed UE list)
        pl.block = pl.big.block;
        pl.grid = (E + pl.big.gpb - 1) / pl.big.gpb;
        pl.lds = (size_t)dcomp::big_carve(B, pl.big.gpb, pl.big.block).total;
        if (pl.lds > 160 * 1024) return fail(DCOMP_EINVAL, "%d UE slots x %d stations do not fit one workgroup's LDS (generic kernel)", CAP, B);
        // multi-agent rows of more than 32 stations: one 16-byte store per lane and row (dcomp_big.h, row loop) once a step's rows no longer sit in
        // the Infinity Cache (measured at 32 x 64: 2 048 envs = 67 MB 41.4 -> 43.1 us, 8 192 = 270 MB 63.9 -> 62.5, 16 384 = 539 MB 196 -> 145,
        // 65 536 = 2.2 GB 693 -> 495); DCOMP_BIG_ROW_X4=0 / 1 forces the four-block form / the 16-byte form
        env->bigp.row_x4 = ovr.big_row_x4.set ? (int32_t)ovr.big_row_x4.v
                                              : ((size_t)E * CAP * row_floats(DCOMP_MULTI, B) * 4 >= ((size_t)128 << 20) ? 1 : 0);
        return DCOMP_OK;
    }
    env->mp_pattern = dcomp::MP_RES_FAIR;      // sharing pattern -> specialised kernel (dcomp_device.h bs_mode_of)
    for (int b = 0; b < B; b++) if (env->kp.bs_mode[b] != DCOMP_RES_FAIR) env->mp_pattern = dcomp::MP_MIXED;
    static const int cyc[3] = {DCOMP_RES_FAIR, DCOMP_RATE_FAIR, DCOMP_PROP_FAIR};   // env_setup.py:40-49
    for (int b = 0; b < B && env->mp_pattern != dcomp::MP_RES_FAIR; b++) if (env->kp.bs_mode[b] != cyc[b % 3]) env->mp_pattern = dcomp::MP_GENERIC;
    const dcomp::KernelPair k = dcomp::lookup_kernels(B, env->upad, env->mp_pattern);
    if (!k.step) return fail(DCOMP_EUNSUPPORTED, "no kernel built for num_bs=%d (built: " DCOMP_B_LIST_STR ")", B);
    // the wide kernel (UPAD >= 64) always uses 256-thread workgroups; the others DCOMP_BLOCK
    const int gpb = DCOMP_BLOCK >= env->upad ? DCOMP_BLOCK / env->upad : 1;
    pl.grid = (E + gpb - 1) / gpb;
    pl.reset = k.reset; pl.step = k.step;
    if (DYN) {                                                    // one launch per step, padded lane groups
        if (!k.step_dyn) return fail(DCOMP_EUNSUPPORTED, "no dynamic-UE kernel for this shape");
        pl.path = StepPath::Dyn; pl.step = k.step_dyn;
        return DCOMP_OK;
    }
    if (k.step_wide && !env->kp.any_maxcap) {
        pl.path = StepPath::Wide; pl.step = k.step_wide;         // one workgroup per slot
        // Batches whose observation rows are >= 1 GB per step -- four times the Infinity Cache: every byte goes out at the sustained HBM
        // write rate -- run with TWO workgroups per CU instead of the four the kernel's 39.8 KB of LDS allow (24 000 B of unused dynamic
        // LDS per workgroup): 16 384 x 128 x 32 252-272 -> 251 us, 32 768 envs 517 -> 477 us (0.60 -> 0.65 of the HBM peak), repeatably;
        // at 8 192 envs (0.54 GB) the same cap costs 6 %, at 4 096 envs (inside the cache) 25 %.  Fewer waves writing at once stream better.
        // Between 0.4 and 1 GB three per CU (13 000 B) are the best of the three: 8 192 envs 141 -> 134 us, 6 144 envs 101.5 -> 98.5 us.
        pl.lds = row_bytes >= 1.0e9 ? 24000 : row_bytes >= 4.0e8 ? 13000 : 0;
        if (ovr.wide_pad_lds.set) pl.lds = (size_t)(int)ovr.wide_pad_lds.v;                         // A/B
        return DCOMP_OK;                                          // never fused, never tight
    }
    // The fused rollout kernel is the LATENCY-optimised variant (state in registers, no LDS staging, no kernel boundaries):
    // it wins while the grid leaves the SIMDs under-occupied (4 096 x 10 x 5: one wave per SIMD, 2.2 vs 5.3 us per step).  A
    // grid of many waves per SIMD is throughput-bound: there the plain step kernel (fewer registers, coalesced staged
    // stores) launched once per step is faster and launch latency hides behind the running kernel.
    // 3 waves per SIMD of the 256 CUs: what the rollout kernel's ~136 VGPRs leave room for (a fourth would wait for a second round)
    const long max_waves = ovr.fuse_max_waves.set ? ovr.fuse_max_waves.v : 3 * 1024;
    const long waves = (long)pl.grid * (DCOMP_BLOCK / 64);
    // Central envs with short rows (2B + 1 <= 17 floats per UE) are faster through the fused kernel at EVERY batch size once a
    // rollout is a few steps long: no kernel boundary (5.4 us per launch, a quarter of a 65 536 x 10 x 5 step), no state round
    // trip, pairs carried from step to step -- 65 536 x 10 x 5: 16.3 vs 19-20 us per step, 16 384: 4.2 vs 11.2, 262 144: 58 vs
    // 63 (T = 50).  Rows of the multi-agent layout (4B + 1 floats per lane, stored straight from registers) stream too
    // badly for that: 65 536 x 32 x 10: 129 vs 77 us.
    // Multi-agent rows (4B + 1 floats per lane) are short enough up to three stations -- the reference's stock small and medium
    // maps: 65 536 x 5 x 3 multi 8.1 vs 12.1 us per step (T = 50); at 10 x 5 it is a draw (23.4 vs 23.3), at 16 x 8 a loss (51.8 vs 38.2).
    if (k.rollout && waves <= max_waves) pl.fuse = Fuse::Always;
    else if (k.rollout && (central ? B <= 8 : B <= 3)) pl.fuse = Fuse::Long;
    // with a registered policy: the variant that carries the rules; tape-driven central envs: the central-only instantiation
    pl.rollout = (central && k.rollout_central) ? k.rollout_central : k.rollout;
    pl.rollout_pol = k.rollout_pol;
    // Tight packing of UE lists whose length is not a power of two (dcomp_device.h, struct Seg): G = U lanes per env,
    // 64 / G envs per wavefront, segmented ds_bpermute reductions (~13 instead of 4 instructions each).  It pays where the
    // launch is throughput-bound and the padding wastes many lanes: >= 4 padded waves per SIMD and >= 1.4x the lanes in use
    // (U = 5, 9, 10, 17-21; measured: 10 x 5 central +10 %, 20 x 10 multi +8 %, 5 x 3 central +14 %, but 12 x 7 multi -2 % at 1.25x).
    // Not with max-cap BSs (their LDS scratch is indexed by padded env slots), not for UE lists that change.
    const int G = CAP, gpw = 64 / G, magic = 65536 / G + 1;
    if (!k.step_tight || G < 3 || (G & (G - 1)) == 0 || env->kp.any_maxcap) return DCOMP_OK;
    const double padded_use = (double)G / env->upad, tight_use = (double)(gpw * G) / 64.0;
    bool want = waves >= 4 * 1024 && tight_use >= 1.4 * padded_use;   // (by itself never together with Fuse::Always: <= 3 * 1024 waves)
    if (ovr.tight.set) want = ovr.tight.v != 0;                       // tests / A-B: force on or off
    for (int l = 0; l < 64; l++) if (((l * magic) >> 16) != l / G) want = false;   // (the kernels divide lane indices by G with this multiplier)
    if (!want) return DCOMP_OK;
    pl.path = StepPath::Tight;
    pl.tight_central = central && k.tight_central;
    pl.step = pl.tight_central ? k.tight_central : k.step_tight;
    pl.lanes = pl.tight_g = G; pl.tight_gpw = gpw; pl.tight_magic = magic;
    pl.tight_grid = (E + gpw * (DCOMP_BLOCK / 64) - 1) / (gpw * (DCOMP_BLOCK / 64));   // gpw envs per wavefront
    // A batch packed tightly for dcomp_step (throughput-bound: >= 4 padded waves per SIMD, >= 1.4x the lanes in use) runs
    // its tape-driven central rollouts tightly packed too: the fused kernel is bound by its VALU work there, and a third fewer
    // waves do the same steps (65 536 x 10 x 5: six envs per wavefront instead of four).  Same packing, same summation order as
    // dcomp_step uses for this env.
    if (central && k.rollout_tight_central) { pl.rollout = k.rollout_tight_central; pl.rollout_tight = true; }
    return DCOMP_OK;
}

static hipError_t upload(void **dst, const void *src, size_t bytes)
{
    hipError_t e = hipMalloc(dst, bytes);
    return e == hipSuccess ? hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) : e;
}
// The handle's device tables; with the generic kernel also its station table and the LDS limit of the kernels the plan launches.
static int upload_tables(dcomp_env *env, const dcomp_cfg *cfg, const std::vector<UeCfg> &uc, const std::vector<double> &vq)
{
    const int U = cfg->num_ue, B = cfg->num_bs;
    hipError_t e = hipSetDevice(cfg->device);
    if (e == hipSuccess) e = upload((void **)&env->d_ue_cfg, uc.data(), sizeof(UeCfg) * U);
    if (e == hipSuccess && !vq.empty()) e = upload((void **)&env->d_ue_velq, vq.data(), sizeof(double) * 2 * U);
    if (e != hipSuccess) return fail(DCOMP_EHIP, "device setup failed: %s", hipGetErrorString(e));
    env->kp.ue_cfg = env->d_ue_cfg; env->kp.ue_velq = env->d_ue_velq;
    if (env->plan.path != StepPath::Generic) return DCOMP_OK;
    const LaunchPlan &pl = env->plan;
    std::vector<double> xy(2 * (size_t)B);
    std::vector<int32_t> md(B);
    for (int b = 0; b < B; b++) { xy[2 * b] = cfg->bs_x[b]; xy[2 * b + 1] = cfg->bs_y[b]; md[b] = cfg->bs_sharing[b]; }
    e = upload((void **)&env->d_bs, xy.data(), sizeof(double) * 2 * B);
    if (e == hipSuccess) e = upload((void **)&env->d_mode, md.data(), sizeof(int32_t) * B);
    for (int pol = 0; pol < 2; pol++)
        for (int c = 0; c < 2; c++)
            for (int w : {pl.big_step, 1, 3})                      // the step this env launches (plain or with events), the reset, the fused rollout
                if (e == hipSuccess) e = raise_lds_limit(reinterpret_cast<const void *>(pl.big.fn[pol][c][w]), (int)pl.lds);
    if (e != hipSuccess) return fail(DCOMP_EHIP, "device setup failed (generic kernel, %zu bytes of LDS per workgroup): %s", pl.lds, hipGetErrorString(e));
    env->bigp.bs = env->d_bs; env->bigp.mode = env->d_mode;
    return DCOMP_OK;
}

extern "C" int dcomp_create_v(int32_t abi_version, size_t cfg_size, size_t state_size, size_t out_size, size_t rollout_opts_size,
                              const dcomp_cfg *cfg, dcomp_env **out)
{
    if (out) *out = nullptr;
    if (abi_version != DCOMP_ABI_VERSION || cfg_size != sizeof(dcomp_cfg) || state_size != sizeof(dcomp_state) || out_size != sizeof(dcomp_out) ||
        rollout_opts_size != sizeof(dcomp_rollout_opts))
        return fail(DCOMP_EABI, "ABI mismatch: caller has version %d, sizeof dcomp_cfg / dcomp_state / dcomp_out / dcomp_rollout_opts = %zu / %zu / %zu / %zu; "
                                "this library has version %d and %zu / %zu / %zu / %zu", (int)abi_version, cfg_size, state_size, out_size, rollout_opts_size,
                    DCOMP_ABI_VERSION, sizeof(dcomp_cfg), sizeof(dcomp_state), sizeof(dcomp_out), sizeof(dcomp_rollout_opts));
    if (!cfg || !out) return fail(DCOMP_EINVAL, "null argument");
    std::vector<UeCfg> uc;
    std::vector<double> vq;
    int rc = validate_cfg(cfg);
    if (!rc) rc = ue_tables(cfg, uc, vq);
    if (rc) return rc;
    std::unique_ptr<dcomp_env, EnvDeleter> env(new dcomp_env());     // every exit below frees it, device tables included
    env->cfg = *cfg;
    env->cfg.bs_x = env->cfg.bs_y = nullptr;   // host arrays are not retained
    env->cfg.ue_pause_duration = env->cfg.ue_border_buffer = nullptr; env->cfg.ue_velocity = nullptr;
    env->ovr = read_overrides();
    env->dyn = cfg->max_ues > 0;               // departures alone need no extra slots: max_ues == num_ue
    env->cap = env->dyn ? cfg->max_ues : cfg->num_ue;
    env->cur_ue = cfg->num_ue;
    env->upad = next_pow2(env->cap) < 4 ? 4 : next_pow2(env->cap);
    if ((rc = fill_constants(env.get(), cfg, uc))) return rc;
    if ((rc = make_plan(env.get()))) return rc;
    if ((rc = upload_tables(env.get(), cfg, uc, vq))) return rc;
    *out = env.release();
    return DCOMP_OK;
}

extern "C" int dcomp_destroy(dcomp_env *env)
{
    if (!env) return DCOMP_OK;
    if (env->d_ue_cfg) (void)hipFree(env->d_ue_cfg);
    if (env->d_ue_velq) (void)hipFree(env->d_ue_velq);
    if (env->d_bs) (void)hipFree(env->d_bs);
    if (env->d_mode) (void)hipFree(env->d_mode);
    delete env;
    return DCOMP_OK;
}

extern "C" int dcomp_state_sizes(const dcomp_env *env, size_t *pos_bytes, size_t *mv_bytes, size_t *conn_bytes, size_t *ewma_bytes,
                                 size_t *flags_bytes, size_t *since_bytes)
{
    if (!env) return fail(DCOMP_EINVAL, "null env");
    size_t n = (size_t)env->cfg.num_envs * env->cap;
    if (pos_bytes) *pos_bytes = n * 16;
    if (mv_bytes) *mv_bytes = n * 8;
    if (conn_bytes) *conn_bytes = n * 4;
    if (ewma_bytes) *ewma_bytes = n * 4;
    if (flags_bytes) *flags_bytes = 16;
    if (since_bytes) *since_bytes = env->kp.any_maxcap ? n * env->cfg.num_bs * 2 : 0;
    return DCOMP_OK;
}

extern "C" int dcomp_obs_dim(const dcomp_env *env, int32_t *floats_per_env, int32_t *reward_per_env)
{
    if (!env) return fail(DCOMP_EINVAL, "null env");
    if (floats_per_env) *floats_per_env = env->cap * row_floats(env->cfg.env_kind, env->cfg.num_bs);
    if (reward_per_env) *reward_per_env = env->cfg.env_kind == DCOMP_MULTI ? env->cap : 1;
    return DCOMP_OK;
}

// Every kernel launch of a handle: `which` kernel of its plan, for either kernel family; the instantiation with / without the in-step
// policy (kp.next_act) and the compact record (kp.obs_compact).  A tightly packed launch gets its packing written into kp.
static void launch(const dcomp_env *env, Launch which, KParams &kp, void *stream)
{
    const LaunchPlan &pl = env->plan;
    if (pl.path == StepPath::Generic) {
        const int w = which == Launch::Reset ? 1 : which == Launch::Rollout ? 3 : pl.big_step;
        hipLaunchKernelGGL(pl.big.fn[kp.next_act ? 1 : 0][kp.obs_compact ? 1 : 0][w], dim3(pl.grid), dim3(pl.block), pl.lds, (hipStream_t)stream, kp, env->bigp);
        return;
    }
    dcomp::KernelFn fn = pl.reset;
    bool tight = false;
    size_t lds = 0;
    if (which == Launch::Step) {
        fn = pl.step;
        tight = pl.path == StepPath::Tight;
        // (the wide kernel's occupancy cap is for launches that stream GBs of ROWS; with the compact record a launch is bound by its arithmetic
        // and wants every wave it can get: 32 768 x 128 x 32 236 us with four workgroups per CU, 369 us with two)
        if (!kp.obs_compact) lds = pl.lds;
    } else if (which == Launch::Rollout) {
        fn = kp.next_act ? pl.rollout_pol : pl.rollout;
        tight = pl.rollout_tight && !kp.next_act;
    }
    if (tight) { kp.tight_g = pl.tight_g; kp.tight_gpw = pl.tight_gpw; kp.tight_magic = pl.tight_magic; }
    hipLaunchKernelGGL(fn, dim3(tight ? pl.tight_grid : pl.grid), dim3(pl.block), lds, (hipStream_t)stream, kp);
}

static int check_horizon(const dcomp_env *env, int steps)
{
    if (env && (int64_t)env->time + steps > 65536)
        return fail(DCOMP_EUNSUPPORTED, "episodes longer than 65536 steps: conn_since and the draw cursor are 16-bit (reset() first)");
    return DCOMP_OK;
}

// One step's departures / arrivals against the `cur` UEs listed before it (base.py:433-443); idx / xy: tape mode's host-drawn list
// positions / border points.  step >= 0: the step of a rollout, named in the message.
static int check_events(const dcomp_env *env, int cur, int nrem, int nadd, const void *idx, const void *xy, int step)
{
    char at[24] = "";
    if (step >= 0) std::snprintf(at, sizeof(at), "step %d: ", step);
    if (nrem < 0 || nadd < 0 || (nrem > 0 && nadd > 0)) return fail(DCOMP_EINVAL, "%sone step either adds or removes UEs (base.py:436-443)", at);
    if (cur - nrem < 1) return fail(DCOMP_EINVAL, "%scannot remove %d of %d UEs", at, nrem, cur);
    if (cur + nadd > env->cap) return fail(DCOMP_EINVAL, "%s%d + %d UEs exceed max_ues = %d", at, cur, nadd, env->cap);
    if (env->cfg.rng_mode == DCOMP_RNG_TAPE && ((nrem && !idx) || (nadd && !xy)))
        return fail(DCOMP_EINVAL, "tape mode: events need the host-drawn indices / border points");
    return DCOMP_OK;
}

static int fill_params(dcomp_env *env, const dcomp_state *st, const dcomp_out *out, KParams &kp)
{
    if (!env || !st || !out) return fail(DCOMP_EINVAL, "null argument");
    if (!st->pos || !st->mv || !st->conn || !st->ewma || !st->flags) return fail(DCOMP_EINVAL, "state pointers must all be set");
    if (!out->obs && !out->obs_compact) return fail(DCOMP_EINVAL, "out->obs (or out->obs_compact) is required");
    if (out->obs_compact) {
        if (out->obs) return fail(DCOMP_EINVAL, "out->obs and out->obs_compact are alternatives: set one, leave the other NULL");
        if (env->cfg.env_kind != DCOMP_MULTI) return fail(DCOMP_EINVAL, "out->obs_compact: the compact record is defined for multi-agent observations (central observations carry no per-env columns)");
    }
    if (env->kp.any_maxcap && !st->conn_since) return fail(DCOMP_EINVAL, "a max-cap BS needs state.conn_since (see dcomp_state_sizes)");
    if (env->plan.path == StepPath::Generic) {
        if (!st->conn_hi) return fail(DCOMP_EINVAL, "more than %d stations: state.conn_hi (stations 32-63 of the connection set, sized like conn) is required", DCOMP_MASK32_MAX_BS);
        env->bigp.conn_hi = st->conn_hi;
    }
    if (env->dyn && !st->uid) return fail(DCOMP_EINVAL, "UE arrival/departure needs state.uid");
    kp = env->kp;
    kp.uid = st->uid;
    kp.orig_consumed = st->orig_consumed;
    kp.cur_ue = env->cur_ue;
    kp.conn_since = st->conn_since;
    kp.time = (uint32_t)env->time;
    kp.pos = (double2 *)st->pos; kp.mv = (unsigned long long *)st->mv; kp.conn = st->conn; kp.ewma = st->ewma; kp.flags = st->flags;
    kp.obs = out->obs_compact ? reinterpret_cast<float *>(out->obs_compact) : out->obs; kp.obs_compact = out->obs_compact ? 1 : 0;
    kp.reward = out->reward; kp.sum_util = out->sum_utility; kp.ue_dr = out->ue_dr; kp.ue_util = out->ue_utility; kp.rb_out = out->reward_before;
    kp.episode = (uint32_t)(env->episode < 0 ? 0 : env->episode);
    kp.num_steps = 1; kp.out_every_step = 0; kp.horizon = 0; kp.episode_inc = 0;
    kp.tight_g = 0; kp.tight_gpw = 0; kp.tight_magic = 0;
    return DCOMP_OK;
}

extern "C" int dcomp_reset(dcomp_env *env, const dcomp_state *st, const dcomp_tape *tape, const dcomp_out *out, void *stream)
{
    KParams kp;
    int rc = fill_params(env, st, out, kp);
    if (rc) return rc;
    if (env->cfg.rng_mode == DCOMP_RNG_TAPE) {
        if (!tape || !tape->pos0 || !tape->triples) return fail(DCOMP_EINVAL, "tape mode: reset needs the episode's draw tape");
        env->kp.tape_pos0 = tape->pos0;                     // borrowed until the next reset
        env->kp.tape_triples = (const ushort4 *)tape->triples;
        env->kp.tape_ids = tape->num_ids > 0 ? tape->num_ids : env->cfg.num_ue;
        kp.tape_pos0 = env->kp.tape_pos0; kp.tape_triples = env->kp.tape_triples; kp.tape_ids = env->kp.tape_ids;
    }
    env->episode += 1;
    env->time = 0;
    env->cur_ue = env->cfg.num_ue; env->n_removed = env->n_arrived = 0;      // base.py:177-182
    kp.cur_ue = env->cur_ue;
    kp.episode = (uint32_t)env->episode;
    launch(env, Launch::Reset, kp, stream);
    HIP_TRY(hipGetLastError());
    return DCOMP_OK;
}

// One step; ev == NULL (dcomp_step): no UE arrives or leaves.
extern "C" int dcomp_step_dyn(dcomp_env *env, const dcomp_state *st, const uint8_t *action, const dcomp_out *out,
                              const dcomp_events *ev, void *stream)
{
    KParams kp;
    int rc = fill_params(env, st, out, kp);
    if (rc) return rc;
    if (!env->dyn) {
        if (ev && (ev->n_remove || ev->n_add)) return fail(DCOMP_EINVAL, "handle was created without max_ues (fixed UE list)");
        ev = nullptr;
    }
    if (!action) return fail(DCOMP_EINVAL, "null action");
    if (env->episode < 0) return fail(DCOMP_EINVAL, "step() before reset()");
    if ((rc = check_horizon(env, 1))) return rc;
    const int nrem = ev ? ev->n_remove : 0, nadd = ev ? ev->n_add : 0;
    if (ev && (rc = check_events(env, env->cur_ue, nrem, nadd, ev->remove_idx, ev->add_xy, -1))) return rc;
    kp.action = action;
    kp.n_remove = nrem; kp.n_add = nadd;
    kp.ev_remove = ev ? ev->remove_idx : nullptr; kp.ev_add_xy = ev ? ev->add_xy : nullptr;
    kp.ev_rem_base = env->n_removed; kp.ev_add_base = env->n_arrived;
    launch(env, Launch::Step, kp, stream);
    HIP_TRY(hipGetLastError());
    env->time += 1;
    env->cur_ue += nadd - nrem;
    env->n_removed += (uint32_t)nrem; env->n_arrived += (uint32_t)nadd;
    return DCOMP_OK;
}
extern "C" int dcomp_step(dcomp_env *env, const dcomp_state *st, const uint8_t *action, const dcomp_out *out, void *stream)
{
    return dcomp_step_dyn(env, st, action, out, nullptr, stream);
}
extern "C" int dcomp_num_ue(const dcomp_env *env) { return env ? env->cur_ue : -1; }

// Whether a rollout of T steps goes through the plan's fused kernel: fusion of the short-row shapes (Fuse::Long) depends on the number
// of steps, and an every-step fragment of >= 2^31 rows does not fit the specialised fused kernel, which addresses step t's outputs as
// (idx + t * E * U) on the caller's base pointers with 32-bit row indices.  Otherwise: one launch per step, same results.
static bool rollout_fused(const dcomp_env *env, int T, bool every, bool loop)
{
    const LaunchPlan &pl = env->plan;
    if (pl.fuse == Fuse::Stretch) return true;                     // (64-bit offsets: no row limit)
    if (every && (uint64_t)T * ((uint64_t)env->cfg.num_envs * env->cap) >= pl.row_limit) return false;
    return pl.fuse == Fuse::Always || (pl.fuse == Fuse::Long && (T >= 4 || loop));
}

// T consecutive steps, in one of three ways: ONE launch of the fused rollout kernel with the horizon inside it (state in registers in
// between); one launch of it per stretch of an episode, the reset kernel in between; one launch of the step kernel per step.  Same
// results either way, and the same as T dcomp_step / dcomp_step_dyn calls (+ dcomp_reset calls at the horizon).
extern "C" int dcomp_rollout_ex(dcomp_env *env, const dcomp_state *st, const uint8_t *actions, int32_t T, const dcomp_out *out,
                                const dcomp_rollout_opts *opts, void *stream)
{
    KParams kp;
    int rc = fill_params(env, st, out, kp);
    if (rc) return rc;
    if (!actions || T < 1) return fail(DCOMP_EINVAL, "bad action tape");
    if (env->episode < 0) return fail(DCOMP_EINVAL, "rollout() before reset()");
    const int L = opts ? opts->horizon : 0, every = opts ? (opts->every_step != 0) : 0;
    const uint32_t inc = (opts && opts->new_episode_draws) ? 1u : 0u;
    const int32_t *ev_rem = opts ? opts->ev_n_remove : nullptr, *ev_add = opts ? opts->ev_n_add : nullptr;
    const int32_t *ev_idx = opts ? opts->ev_remove_idx : nullptr, *ev_xy = opts ? opts->ev_add_xy : nullptr;
    const bool tape = env->cfg.rng_mode == DCOMP_RNG_TAPE;
    if (L < 0 || L > 65536) return fail(DCOMP_EINVAL, "horizon must be 0 (none) .. 65536");
    if (L > 0) {
        if (env->time > L) return fail(DCOMP_EINVAL, "env.time %d is already beyond the horizon %d", env->time, L);
        if (tape && inc) return fail(DCOMP_EINVAL, "tape mode replays the borrowed tape: only fixed episodes can reset inside a rollout");
        if (tape && env->dyn) return fail(DCOMP_EUNSUPPORTED, "tape mode with UE arrival / departure: every episode needs its own host-drawn tape "
                                                              "(the reference re-seeds UEs by list position at reset, base.py:171-173); dcomp_reset between rollouts");
    } else if ((rc = check_horizon(env, T))) return rc;
    if (!env->dyn && (ev_rem || ev_add)) return fail(DCOMP_EINVAL, "handle was created without max_ues (fixed UE list): no arrival / departure events");
    const bool loop = opts && opts->policy_loop != 0;
    if (loop && !env->kp.next_act) return fail(DCOMP_EINVAL, "policy_loop needs a policy (dcomp_set_policy)");
    const size_t EU = (size_t)env->cfg.num_envs * env->cap, E = (size_t)env->cfg.num_envs;
    const bool multi = env->cfg.env_kind == DCOMP_MULTI;
    const size_t obs_step = EU * (size_t)row_floats(env->cfg.env_kind, env->cfg.num_bs);
    auto out_slice = [&](KParams &k, int t) {                  // where step t's outputs go
        if (!every) return;
        k.obs = out->obs_compact ? reinterpret_cast<float *>(out->obs_compact) + E * (size_t)dcomp_frag::env_words(env->cap, env->cfg.num_bs) * t
                                 : out->obs + obs_step * t;
        if (out->reward) k.reward = out->reward + (multi ? EU : E) * t;
        if (out->sum_utility) k.sum_util = out->sum_utility + E * t;
        if (out->ue_dr) k.ue_dr = out->ue_dr + EU * t;
        if (out->ue_utility) k.ue_util = out->ue_utility + EU * t;
        if (out->reward_before) k.rb_out = out->reward_before + EU * t;
    };
    auto launch_reset = [&](KParams &k) {                      // MobileEnv.reset at the horizon (base.py:169-189); its observation lands
        env->time = 0;                                         // where the next step's will (and is overwritten by it)
        env->episode += tape ? 1 : inc;                        // (tape mode: `episode` counts resets, as dcomp_reset does; the draws do not use it)
        env->cur_ue = env->cfg.num_ue; env->n_removed = env->n_arrived = 0;
        k.cur_ue = env->cur_ue;
        k.episode = (uint32_t)env->episode;
        k.time = 0u;
        launch(env, Launch::Reset, k, stream);
    };
    if (env->dyn) {
        // The whole schedule is validated BEFORE the first launch: the call enqueues all T steps or nothing (an invalid entry at step t
        // must not leave the env t steps advanced and the caller's event streams consumed).
        int cur = env->cur_ue, time = env->time;
        for (int t = 0; t < T; t++) {
            if (L > 0 && time == L) { time = 0; cur = env->cfg.num_ue; }
            const int nrem = ev_rem ? ev_rem[t] : 0, nadd = ev_add ? ev_add[t] : 0;
            if ((rc = check_events(env, cur, nrem, nadd, ev_idx, ev_xy, t))) return rc;
            cur += nadd - nrem;
            time += 1;
        }
    }
    // The closed loop: step 0 acts on actions[0] (the next_action the previous launch wrote), every later step -- and the first step of a
    // new episode, on the reset kernel's observation -- on what the launch before it decided.  next_action is ONE buffer read and written
    // in place: a lane reads the action of its own slot when the kernel starts and writes the decision for that same slot at its end (with
    // UE arrival / departure the UEs move between slots through LDS, not through this buffer).
    const uint8_t *act_src = actions;
    if (rollout_fused(env, T, every, loop)) {
        if (env->plan.fuse != Fuse::Stretch && (!loop || L == 0 || env->time + T <= L)) {
            // ONE launch; resets at the horizon of a tape-driven rollout happen inside the kernel
            kp.action = actions; kp.num_steps = T; kp.out_every_step = every; kp.horizon = L; kp.episode_inc = inc; kp.policy_loop = loop;
            launch(env, Launch::Rollout, kp, stream);
            for (int t = 0; t < T; t++) {
                if (L > 0 && env->time == L) { env->time = 0; env->episode += tape ? 1 : inc; }
                env->time += 1;
            }
        } else {
            // One launch per stretch of an episode (the generic kernel; the specialised one in a closed loop that crosses episode
            // boundaries); at the horizon the reset kernel, which with a policy also decides the first action of the new episode.
            for (int t = 0; t < T;) {
                out_slice(kp, t);
                if (L > 0 && env->time == L) { launch_reset(kp); if (loop) act_src = kp.next_act; }
                const int n = (L > 0 && L - env->time < T - t) ? L - env->time : T - t;
                kp.action = loop ? act_src : actions + EU * t;
                kp.num_steps = n; kp.out_every_step = every; kp.policy_loop = loop; kp.horizon = 0; kp.episode_inc = 0;
                kp.time = (uint32_t)env->time; kp.episode = (uint32_t)env->episode;
                launch(env, Launch::Rollout, kp, stream);
                env->time += n;
                t += n;
                if (loop) act_src = kp.next_act;                   // (a lane reads its slot before it writes it)
            }
        }
        HIP_TRY(hipGetLastError());
        return DCOMP_OK;
    }
    size_t rem_off = 0, add_off = 0;
    for (int t = 0; t < T; t++) {
        out_slice(kp, t);
        if (L > 0 && env->time == L) { launch_reset(kp); if (loop) act_src = kp.next_act; }
        kp.episode = (uint32_t)env->episode;
        kp.action = loop ? act_src : actions + EU * t;
        kp.time = (uint32_t)env->time;
        kp.n_remove = kp.n_add = 0;
        if (env->dyn) {                                            // base.py:433-443: this step's departures / arrivals
            const int nrem = ev_rem ? ev_rem[t] : 0, nadd = ev_add ? ev_add[t] : 0;       // (validated above, all T steps)
            kp.cur_ue = env->cur_ue;
            kp.n_remove = nrem; kp.n_add = nadd;
            kp.ev_remove = (tape && nrem) ? ev_idx + rem_off : nullptr;
            kp.ev_add_xy = (tape && nadd) ? ev_xy + add_off : nullptr;
            kp.ev_rem_base = env->n_removed; kp.ev_add_base = env->n_arrived;
            rem_off += E * (size_t)nrem; add_off += E * (size_t)nadd * 2;
            env->cur_ue += nadd - nrem;
            env->n_removed += (uint32_t)nrem; env->n_arrived += (uint32_t)nadd;
        }
        launch(env, Launch::Step, kp, stream);
        env->time += 1;
        if (loop) act_src = kp.next_act;
    }
    HIP_TRY(hipGetLastError());
    return DCOMP_OK;
}

extern "C" int dcomp_rollout(dcomp_env *env, const dcomp_state *st, const uint8_t *actions, int32_t num_steps, const dcomp_out *out,
                             void *stream)
{
    return dcomp_rollout_ex(env, st, actions, num_steps, out, nullptr, stream);
}

extern "C" int dcomp_rollout_is_fused(const dcomp_env *env) { return env ? (env->plan.fuse != Fuse::None ? 1 : 0) : -1; }
extern "C" int dcomp_rollout_fused_for(const dcomp_env *env, int32_t num_steps, int32_t every_step, int32_t policy_loop)
{
    if (!env || num_steps < 1) return -1;
    return rollout_fused(env, num_steps, every_step != 0, policy_loop != 0) ? 1 : 0;
}
// 1: this env runs on the generic kernel, whose connection sets take two words per UE -- dcomp_state.conn_hi is REQUIRED (dcomp_reset / dcomp_step
// fail with DCOMP_EINVAL without it); 0: the specialised kernels, conn_hi is ignored.  The caller asks instead of re-deriving the rule.
extern "C" int dcomp_needs_conn_hi(const dcomp_env *env) { return env ? (env->plan.path == StepPath::Generic ? 1 : 0) : -1; }
extern "C" int dcomp_lanes_per_env(const dcomp_env *env) { return env ? env->plan.lanes : -1; }

// The instantiation dcomp_step launches for this env, spelled as rocprofv3 prints it ("step_kernel<10, 32, 2>"): bench.py ties a
// tracked --pmc profile to the kernel the library really dispatches to.
extern "C" int dcomp_step_kernel_name(const dcomp_env *env, char *buf, int32_t len)
{
    if (!env || !buf || len < 1) return fail(DCOMP_EINVAL, "null argument");
    const int B = env->cfg.num_bs, W = env->upad, MP = env->mp_pattern;
    switch (env->plan.path) {
    case StepPath::Generic: std::snprintf(buf, (size_t)len, "big_kernel<%d, false, %s, false, %s, false>", W, env->dyn ? "true" : "false", env->kp.next_act ? "true" : "false"); break;
    case StepPath::Tight: std::snprintf(buf, (size_t)len, "step_kernel_tight<%d, %d, %d, %d>", B, W, MP, env->plan.tight_central ? 0 : -1); break;
    case StepPath::Dyn: std::snprintf(buf, (size_t)len, "step_kernel_dyn<%d, %d, %d>", B, W, MP); break;
    case StepPath::Wide: std::snprintf(buf, (size_t)len, "step_kernel_wide<%d, %d, %d>", B, W, MP); break;
    case StepPath::Special: std::snprintf(buf, (size_t)len, "step_kernel<%d, %d, %d>", B, W, MP); break;
    }
    return DCOMP_OK;
}

extern "C" int dcomp_check(dcomp_env *env, const dcomp_state *st, void *stream)
{
    if (!env || !st || !st->flags) return fail(DCOMP_EINVAL, "null argument");
    uint32_t h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, st->flags, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (h[0]) HIP_TRY(hipMemsetAsync(st->flags, 0, sizeof(h), (hipStream_t)stream));
    if (h[0] & DCOMP_FLAG_BAD_ACTION) return fail(DCOMP_EACTION, "an action does not fit the action space [0, %d]", env->cfg.num_bs);
    if (h[0] & DCOMP_FLAG_TAPE_EMPTY) return fail(DCOMP_ETAPE, "waypoint draw tape exhausted (depth %d)", env->cfg.tape_depth);
    if (h[0] & DCOMP_FLAG_OUTSIDE_MAP) return fail(DCOMP_EPOS, "a UE position is outside the map");
    return DCOMP_OK;
}

extern "C" int dcomp_time(const dcomp_env *env) { return env ? env->time : -1; }
extern "C" int64_t dcomp_episode(const dcomp_env *env) { return env ? env->episode : -1; }
extern "C" int dcomp_get_counters(const dcomp_env *env, int64_t out[5])
{
    if (!env || !out) return fail(DCOMP_EINVAL, "null argument");
    out[0] = env->time; out[1] = env->episode; out[2] = env->cur_ue; out[3] = env->n_removed; out[4] = env->n_arrived;
    return DCOMP_OK;
}
extern "C" int dcomp_set_counters(dcomp_env *env, const int64_t in[5])
{
    if (!env || !in) return fail(DCOMP_EINVAL, "null argument");
    if (in[0] < 0 || in[1] < -1 || in[2] < 1 || in[2] > env->cap || in[3] < 0 || in[4] < 0) return fail(DCOMP_EINVAL, "counters out of range");
    if (!env->dyn && (in[2] != env->cfg.num_ue || in[3] || in[4])) return fail(DCOMP_EINVAL, "fixed UE list: num_ue / event counters cannot change");
    env->time = (int)in[0]; env->episode = in[1]; env->cur_ue = (int)in[2];
    env->n_removed = (uint32_t)in[3]; env->n_arrived = (uint32_t)in[4];
    return DCOMP_OK;
}
extern "C" int dcomp_set_seed(dcomp_env *env, uint64_t seed)
{
    if (!env) return fail(DCOMP_EINVAL, "null env");
    env->cfg.seed = seed;
    env->kp.seed_lo = (uint32_t)seed; env->kp.seed_hi = (uint32_t)(seed >> 32);
    return DCOMP_OK;
}
extern "C" int dcomp_set_tape(dcomp_env *env, const dcomp_tape *tape, int32_t depth)
{
    if (!env || !tape || !tape->pos0 || !tape->triples) return fail(DCOMP_EINVAL, "null argument");
    if (env->cfg.rng_mode != DCOMP_RNG_TAPE) return fail(DCOMP_EINVAL, "handle draws with Philox: it has no tape");
    if (depth < env->cfg.tape_depth) return fail(DCOMP_EINVAL, "the replacement tape (depth %d) must contain the current one (depth %d)", depth, env->cfg.tape_depth);
    const int ids = tape->num_ids > 0 ? tape->num_ids : env->cfg.num_ue;
    if (env->episode >= 0 && ids != env->kp.tape_ids) return fail(DCOMP_EINVAL, "tape has %d streams per env, the episode was started with %d", ids, env->kp.tape_ids);
    env->cfg.tape_depth = depth;
    env->kp.tape_depth = depth;
    env->kp.tape_pos0 = tape->pos0;
    env->kp.tape_triples = (const ushort4 *)tape->triples;
    env->kp.tape_ids = ids;
    return DCOMP_OK;
}
extern "C" int dcomp_set_episode(dcomp_env *env, int64_t episode)
{
    if (!env) return fail(DCOMP_EINVAL, "null env");
    env->episode = episode - 1;     // the next reset() starts `episode`
    return DCOMP_OK;
}

// ---------------------------------------------------------------------------------------------------------
// CPython-compatible MT19937: random.Random(int).randint(a, b)   (stdlib: Modules/_randommodule.c, Lib/random.py)
namespace {
struct PyMT {
    uint32_t mt[624];
    int idx;
    void init_genrand(uint32_t s)
    {
        mt[0] = s;
        for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        idx = 624;
    }
    void init_by_array(const uint32_t *key, int len)
    {
        init_genrand(19650218u);
        int i = 1, j = 0;
        for (int k = (624 > len ? 624 : len); k; k--) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
            i++; j++;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
            if (j >= len) j = 0;
        }
        for (int k = 623; k; k--) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
            i++;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
        }
        mt[0] = 0x80000000u;
    }
    void seed(int64_t s)
    {   // random.seed(int): key = 32-bit little-endian digits of abs(s)
        uint64_t a = (uint64_t)(s < 0 ? -s : s);
        uint32_t key[2] = {(uint32_t)a, (uint32_t)(a >> 32)};
        init_by_array(key, key[1] ? 2 : 1);
    }
    uint32_t next()
    {
        if (idx >= 624) {
            int kk;
            for (kk = 0; kk < 624 - 397; kk++) { uint32_t y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu); mt[kk] = mt[kk + 397] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u); }
            for (; kk < 623; kk++) { uint32_t y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu); mt[kk] = mt[kk + (397 - 624)] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u); }
            uint32_t y = (mt[623] & 0x80000000u) | (mt[0] & 0x7fffffffu);
            mt[623] = mt[396] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= (y >> 11); y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= (y >> 18);
        return y;
    }
    uint32_t randbelow(uint32_t n)
    {   // Random._randbelow_with_getrandbits: k = n.bit_length(); r = getrandbits(k) until r < n
        int k = 32 - __builtin_clz(n);
        uint32_t r = next() >> (32 - k);
        while (r >= n) r = next() >> (32 - k);
        return r;
    }
    int randint(int a, int b) { return a + (int)randbelow((uint32_t)(b - a + 1)); }
};
}  // namespace

extern "C" int dcomp_mt_draw_tape(const dcomp_cfg *cfg, const int64_t *seeds, int32_t num_envs, int32_t depth, int32_t *pos0,
                                  uint16_t *triples)
{
    if (!cfg || !seeds || !pos0 || !triples || depth < 1 || num_envs < 1) return fail(DCOMP_EINVAL, "bad argument");
    const int U = cfg->num_ue, W = cfg->map_w, H = cfg->map_h;
    if (!cfg->ue_vel_lo || !cfg->ue_vel_hi) return fail(DCOMP_EINVAL, "velocity ranges required");
    auto work = [&](int e0, int e1) {
    for (int e = e0; e < e1; e++) {
        PyMT pos_rng, mov_rng;
        for (int u = 0; u < U; u++) {
            const int64_t s = seeds[e] + 100 * (int64_t)(u + 1);     // base.py:138-143
            pos_rng.seed(s); mov_rng.seed(s);                        // user.py:94-96 (same seed for both streams)
            const size_t idx = (size_t)e * U + u;
            const int ix = cfg->ue_init_x ? cfg->ue_init_x[u] : -1, iy = cfg->ue_init_y ? cfg->ue_init_y[u] : -1;
            pos0[2 * idx] = ix < 0 ? pos_rng.randint(0, W) : ix;                 // user.py:102-103
            pos0[2 * idx + 1] = iy < 0 ? pos_rng.randint(0, H) : iy;             // user.py:106-107
            for (int k = 0; k < depth; k++) {
                const int lo = cfg->ue_vel_lo[u], hi = cfg->ue_vel_hi[u];
                uint16_t *t = triples + (idx * depth + k) * 4;
                t[0] = (uint16_t)(lo != hi ? mov_rng.randint(lo, hi) : lo);      // movement.py:112-117
                const int bb = cfg->ue_border_buffer ? cfg->ue_border_buffer[u] : 10;
                t[1] = (uint16_t)mov_rng.randint(bb, W - bb);                    // movement.py:126
                t[2] = (uint16_t)mov_rng.randint(bb, H - bb);                    // movement.py:127
                t[3] = 0;
            }
        }
    }
    };
    unsigned nt = std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > 32) nt = 32;
    if ((int64_t)num_envs * U < 4096) nt = 1;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) {
        int e0 = (int)((int64_t)num_envs * t / nt), e1 = (int)((int64_t)num_envs * (t + 1) / nt);
        if (e1 > e0) th.emplace_back(work, e0, e1);
    }
    for (auto &t : th) t.join();
    return DCOMP_OK;
}

// ---------------------------------------------------------------------------------------------------------
// heuristic baselines (deepcomp/agent/heuristics.py) on the packed observation tensor
namespace {
struct PolicyParams {
    int policy, multi, U, B, active;
    int aligned;                  // obs is 16-byte aligned (multi-agent layout: float4 loads)
    int64_t rows;                 // E * U
    float eps;
    const uint32_t *cluster;
};

// One lane per (env, UE).  A wave first copies its 64 rows into LDS with consecutive lanes on consecutive addresses (per-lane
// row reads would touch 64 cache lines per load instruction).  Multi-agent layout: the 64 rows of 4B+1 floats are ONE
// contiguous, 256-byte aligned span -> 16-byte loads of the whole span (the ues_at_bs | util_at_bs half the rules do not read
// shares its cache lines with connected | dr, so skipping it would not save HBM traffic); central layout (small tensors):
// the connected and dr runs of each row, float by float.  Row stride in LDS 4B+1 / 2B+1 words: odd = conflict-free per-lane walks.
__global__ void __launch_bounds__(256) heuristic_kernel(PolicyParams p, const float *__restrict__ obs, uint8_t *__restrict__ act)
{
    extern __shared__ float4 lds4[];
    float *const lds = reinterpret_cast<float *>(lds4);
    const int B = p.B, W = 2 * B, S = p.multi ? 4 * B + 1 : W + 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    float *buf = lds + wave * 64 * S;
    const int64_t r0 = ((int64_t)blockIdx.x * wpb + wave) * 64;
    const int64_t left = p.rows - r0;
    const int nrows = left >= 64 ? 64 : left > 0 ? (int)left : 0;
    if (p.multi) {                                                     // connected[B] | dr[B] lead the row (variants.py:255-269)
        const float *src = obs + r0 * S;
        const int nfl = nrows * S;
        const int nq = p.aligned ? nfl >> 2 : 0;
        typedef float f4 __attribute__((ext_vector_type(4)));
        const f4 *src4 = reinterpret_cast<const f4 *>(src);
        for (int q0 = lane; q0 < nq; q0 += 64 * 16) {                  // 16 loads in flight per lane, then the LDS stores
            f4 v[16];
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] = q0 + 64 * k < nq ? __builtin_nontemporal_load(src4 + q0 + 64 * k) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 16; k++) if (q0 + 64 * k < nq) reinterpret_cast<f4 *>(buf)[q0 + 64 * k] = v[k];
        }
        for (int i0 = 4 * nq + lane; i0 < nfl; i0 += 64 * 8) {         // tail / unaligned tensor: float by float
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = i0 + 64 * k < nfl ? src[i0 + 64 * k] : 0.f;
#pragma unroll
            for (int k = 0; k < 8; k++) if (i0 + 64 * k < nfl) buf[i0 + 64 * k] = v[k];
        }
    } else {                                                           // connected[U*B] | dr[U*B] | utility[U] (central.py:147-151)
        const int64_t env_floats = (int64_t)p.U * (W + 1);
        for (int i0 = lane; i0 < nrows * W; i0 += 64 * 8) {
            float v[8];
            int at[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = i0 + 64 * k;
                const int row = i / W, col = i - row * W;
                const int64_t r = r0 + row;
                const int64_t e = r / p.U;
                const int u = (int)(r - e * p.U);
                at[k] = row * S + col;
                v[k] = i < nrows * W ? obs[e * env_floats + (col < B ? u * B + col : p.U * B + u * B + col - B)] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 8; k++) if (i0 + 64 * k < nrows * W) buf[at[k]] = v[k];
        }
    }
    __syncthreads();
    if (lane >= nrows) return;
    const float *row = buf + lane * S;
    const int64_t r = r0 + lane;
    const int u = (int)(r % p.U);
    unsigned long long conn = 0;                                       // (64-bit sets: up to 64 stations, round 5)
    float mx = -__builtin_huge_valf();
    int best = 0;
#pragma unroll 8
    for (int b = 0; b < B; b++) {
        conn |= (row[b] > 0.5f ? 1ull : 0ull) << b;
        const float d = row[B + b];
        if (d > mx) { mx = d; best = b; }                              // strict: the first maximum (np.argmax, heuristics.py:27)
    }
    int a = 0;
    if (u >= p.active) a = 0;
    else if (p.policy == DCOMP_POLICY_3GPP) {
        if ((conn >> best) & 1ull) a = 0;                              // heuristics.py:30-31: already at the best cell
        else if (conn) a = __builtin_ffsll((long long)conn);           // :33-36: drop the (first) other connection
        else a = best + 1;                                             // :38
    } else {
        unsigned long long sel = B == 64 ? ~0ull : (1ull << B) - 1ull; // FullCoMP: every cell
        if (p.policy == DCOMP_POLICY_DYNAMIC) {
            const float thr = mx * p.eps;                              // heuristics.py:87-90
            sel = 0;
#pragma unroll 8
            for (int b = 0; b < B; b++) sel |= (row[B + b] >= thr ? 1ull : 0ull) << b;
        } else if (p.policy == DCOMP_POLICY_CLUSTER)                   // :172-176; one word per station up to 32 stations, two (lo, hi) beyond
            sel = B <= 32 ? (unsigned long long)p.cluster[best] : ((unsigned long long)p.cluster[2 * best] | ((unsigned long long)p.cluster[2 * best + 1] << 32));
        const unsigned long long drop = conn & ~sel;
        if (drop) a = __builtin_ffsll((long long)drop);                // :96-99 / :178-181: index order
        else {
            const unsigned long long cand = sel & ~conn;
            float m2 = -__builtin_huge_valf();
#pragma unroll 8
            for (int b = 0; b < B; b++) {
                const float d = row[B + b];
                if (((cand >> b) & 1ull) && d > m2) { m2 = d; a = b + 1; }   // strongest first, first of equals (:57-63, :101-106)
            }
        }
    }
    act[r] = (uint8_t)a;
}
}  // namespace

extern "C" int dcomp_set_policy(dcomp_env *env, const dcomp_policy *p, uint8_t *next_action)
{
    if (!env) return fail(DCOMP_EINVAL, "null argument");
    if (!p || !next_action) { env->kp.next_act = nullptr; return DCOMP_OK; }
    if (p->policy < DCOMP_POLICY_3GPP || p->policy > DCOMP_POLICY_CLUSTER) return fail(DCOMP_EINVAL, "unknown policy %d", p->policy);
    if ((p->num_envs && p->num_envs != env->cfg.num_envs) || (p->num_ue && p->num_ue != env->kp.U) || (p->num_bs && p->num_bs != env->cfg.num_bs))
        return fail(DCOMP_EINVAL, "policy shape (%d, %d, %d) is not the env's (%d, %d, %d)", p->num_envs, p->num_ue, p->num_bs,
                    env->cfg.num_envs, env->kp.U, env->cfg.num_bs);
    if (p->policy == DCOMP_POLICY_CLUSTER && !p->cluster_mask) return fail(DCOMP_EINVAL, "DCOMP_POLICY_CLUSTER needs cluster_mask");
    if (p->policy == DCOMP_POLICY_DYNAMIC && !(p->epsilon >= 0.f && p->epsilon <= 1.f)) return fail(DCOMP_EINVAL, "epsilon must be in [0, 1]");
    env->kp.policy = p->policy; env->kp.policy_eps = p->epsilon; env->kp.policy_cluster = p->cluster_mask;
    env->kp.next_act = next_action;
    return DCOMP_OK;
}

extern "C" int dcomp_heuristic_actions(const dcomp_policy *p, const float *obs, uint8_t *action, void *stream)
{
    if (!p || !obs || !action) return fail(DCOMP_EINVAL, "null argument");
    if (p->num_envs < 1 || p->num_ue < 1 || p->num_ue > DCOMP_MAX_UE || p->num_bs < 1 || p->num_bs > DCOMP_MAX_BS)
        return fail(DCOMP_EINVAL, "need num_envs>=1, 1<=num_ue<=%d, 1<=num_bs<=%d (got %d, %d, %d)", DCOMP_MAX_UE, DCOMP_MAX_BS, p->num_envs, p->num_ue, p->num_bs);
    if (p->policy < DCOMP_POLICY_3GPP || p->policy > DCOMP_POLICY_CLUSTER) return fail(DCOMP_EINVAL, "unknown policy %d", p->policy);
    if (p->obs_kind != DCOMP_CENTRAL && p->obs_kind != DCOMP_MULTI) return fail(DCOMP_EINVAL, "obs_kind must be DCOMP_CENTRAL or DCOMP_MULTI");
    if (p->num_active < 0 || p->num_active > p->num_ue) return fail(DCOMP_EINVAL, "num_active (%d) outside [0, num_ue]", p->num_active);
    if (p->policy == DCOMP_POLICY_CLUSTER && !p->cluster_mask) return fail(DCOMP_EINVAL, "DCOMP_POLICY_CLUSTER needs cluster_mask");
    if (p->policy == DCOMP_POLICY_DYNAMIC && !(p->epsilon >= 0.f && p->epsilon <= 1.f)) return fail(DCOMP_EINVAL, "epsilon must be in [0, 1]");
    PolicyParams k;
    k.policy = p->policy; k.multi = p->obs_kind == DCOMP_MULTI; k.U = p->num_ue; k.B = p->num_bs; k.active = p->num_active;
    k.rows = (int64_t)p->num_envs * p->num_ue; k.eps = p->epsilon; k.cluster = p->cluster_mask;
    k.aligned = (reinterpret_cast<uintptr_t>(obs) & 15u) == 0;
    const size_t per_wave = (size_t)64 * ((k.multi ? 4 : 2) * p->num_bs + 1) * sizeof(float);
    int wpb = (int)(60 * 1024 / per_wave);
    wpb = wpb > 4 ? 4 : wpb < 1 ? 1 : wpb;
    if (per_wave * wpb > 64 * 1024) {           // 64 rows of more than 60 stations: one wave per workgroup, above the default 64 KiB of dynamic LDS
        HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(heuristic_kernel), 72 * 1024));
    }
    const int64_t waves = (k.rows + 63) / 64;
    dim3 grid((unsigned)((waves + wpb - 1) / wpb)), block(64 * wpb);
    hipLaunchKernelGGL(heuristic_kernel, grid, block, per_wave * wpb, (hipStream_t)stream, k, obs, action);
    HIP_TRY(hipGetLastError());
    return DCOMP_OK;
}

// ---------------------------------------------------------------------------------------------------------
// device self-tests
namespace {
__global__ void selftest_fp64(int op, const double *x, const double *y, double *out, int64_t n)
{
#pragma clang fp contract(off)
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a = x[i], b = y[i], r;
    if (op == 0) r = __builtin_sqrt(a);
    else if (op == 1) r = a / b;
    else if (op == 2) r = __builtin_fma(b, b, a * a);
    else {                                             // 4, 5, 6: move_ue's norm_and_unit(vx = x, vy = y) -> nrm, nx, ny
        double nrm, nx, ny;
        dcomp::norm_and_unit(a, b, nrm, nx, ny);
        r = op == 4 ? nrm : op == 5 ? nx : ny;
    }
    out[i] = r;
}
template <int W>
__global__ void selftest_reduce(const double *x, double *out, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float v = i < n ? (float)x[i] : 0.f;
    float s = dcomp::group_reduce<W, dcomp::OpSum>(v);
    float m = dcomp::group_reduce<W, dcomp::OpMin>(v);
    int lane = threadIdx.x & 63;
    int c = dcomp::group_count<W>(v > 0.f, lane & ~(W - 1));
    if (i < n) out[i] = (double)s + 1024.0 * (double)c + 1048576.0 * (double)m;
}
}  // namespace

extern "C" int dcomp_selftest(int op, int width, const double *x, const double *y, double *out, int64_t n, void *stream)
{
    if (!x || !out || n < 1) return fail(DCOMP_EINVAL, "bad argument");
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if ((op >= 0 && op <= 2) || (op >= 4 && op <= 6)) {
        if (!y) return fail(DCOMP_EINVAL, "y required");
        hipLaunchKernelGGL(selftest_fp64, grid, block, 0, s, op, x, y, out, n);
    } else if (op == 3) {
        switch (width) {
        case 2: hipLaunchKernelGGL(selftest_reduce<2>, grid, block, 0, s, x, out, n); break;
        case 4: hipLaunchKernelGGL(selftest_reduce<4>, grid, block, 0, s, x, out, n); break;
        case 8: hipLaunchKernelGGL(selftest_reduce<8>, grid, block, 0, s, x, out, n); break;
        case 16: hipLaunchKernelGGL(selftest_reduce<16>, grid, block, 0, s, x, out, n); break;
        case 32: hipLaunchKernelGGL(selftest_reduce<32>, grid, block, 0, s, x, out, n); break;
        case 64: hipLaunchKernelGGL(selftest_reduce<64>, grid, block, 0, s, x, out, n); break;
        default: return fail(DCOMP_EINVAL, "width must be 2..64 (power of two)");
        }
    } else return fail(DCOMP_EINVAL, "unknown op");
    HIP_TRY(hipGetLastError());
    return DCOMP_OK;
}

// ---- compact rollout fragments for the learner hand-off (dcomp_fragment.h) ----
extern "C" int dcomp_fragment_words(int32_t num_ue, int32_t num_bs)
{
    if (num_ue < 1 || num_ue > DCOMP_MAX_UE || num_bs < 1 || num_bs > DCOMP_MAX_BS) return -1;    // (round 6: two mask words per UE with more than 32 stations)
    return dcomp_frag::env_words(num_ue, num_bs);
}

static int fragment_params(dcomp_frag::FragParams &p, int64_t n, int U, int B, int &grid, size_t &lds_pack, size_t &lds_unpack)
{
    if (n < 1 || U < 1 || U > DCOMP_MAX_UE || B < 1 || B > DCOMP_MAX_BS)
        return fail(DCOMP_EINVAL, "fragment: need num_env_steps >= 1, 1 <= num_ue <= %d, 1 <= num_bs <= %d", DCOMP_MAX_UE, DCOMP_MAX_BS);
    if (dcomp_frag::fill(p, n, U, B, grid, lds_pack, lds_unpack)) return fail(DCOMP_EINVAL, "fragment too long for one launch: split it (num_env_steps * chunks >= 2^31)");
    return DCOMP_OK;
}

extern "C" int dcomp_pack_fragment(const float *obs, int64_t num_env_steps, int32_t num_ue, int32_t num_bs, uint32_t *packed, int32_t *flags,
                                   void *stream)
{
    if (!obs || !packed || !flags) return fail(DCOMP_EINVAL, "null argument");
    dcomp_frag::FragParams p{};
    int grid;
    size_t lp, lu;
    const int rc = fragment_params(p, num_env_steps, num_ue, num_bs, grid, lp, lu);
    if (rc) return rc;
    p.obs_in = obs; p.packed_out = packed; p.flags = flags;
    hipLaunchKernelGGL(dcomp_frag::pack_kernel, dim3(grid), dim3(dcomp_frag::BLOCK), lp, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DCOMP_OK;
}

extern "C" int dcomp_unpack_fragment(const uint32_t *packed, int64_t num_env_steps, int32_t num_ue, int32_t num_bs, float *obs, void *stream)
{
    if (!obs || !packed) return fail(DCOMP_EINVAL, "null argument");
    dcomp_frag::FragParams p{};
    int grid;
    size_t lp, lu;
    const int rc = fragment_params(p, num_env_steps, num_ue, num_bs, grid, lp, lu);
    if (rc) return rc;
    p.packed_in = packed; p.obs_out = obs;
    hipLaunchKernelGGL(dcomp_frag::unpack_kernel, dim3(grid), dim3(dcomp_frag::BLOCK), lu, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DCOMP_OK;
}
