// dcomp_gae_uid.hip -- advantages that follow a UE through the slots of a dynamic env by its uid word (include/dcomp_gae_uid.h has the
// semantics and what a trace may be assumed to be).  An object of its own: it shares no kernel code with the others.
//
// Lanes are slots.  Every lane walks t backwards and holds the carry (nv, A) = (value, advantage) of ITS slot in the layout after step
// t (uid_next[t]'s).  Per step a lane looks its own word uid[t][e][s] up in uid_next[t][e][s, s-1, ..., s-scan] -- survivors only ever
// move up -- and fetches the reward and the carry from the slot s' where it found it; then the f32 operations of gae_kernel
// (dcomp_actor.hip) in its order.  A row whose word is 0 or not found does not count: it writes zeros and carries (0, 0), which is what
// ends the trajectory of the UE that had this slot before the departure.  The fetch is
//   U <= 64: __shfl inside the env's group of UPAD lanes (UPAD the power of two >= U, 64 / UPAD envs per wavefront), no LDS, no barrier;
//   U  > 64: one workgroup of ceil(U / 64) wavefronts per env; uid_next[t]'s row, the rewards and the carry are published in LDS, with a
//            barrier between publish and read and another before the next publish (DynExchange in dcomp_dyn.h is the model).
// The t loop, end[t] and the env loops are uniform per wavefront (per workgroup in the wide kernel): every lane reaches every shuffle and
// every barrier.  Values of rows that do not count are only ever SELECTED away, never multiplied by 0: a NaN there reaches no output.
// All accesses are element-wide (2-byte words of a row of odd U start at a 2-byte phase).
#include "dcomp_actor_impl.h"                 // host helpers only: fail, HIP_TRY, check_struct
#include "../../include/dcomp_gae_uid.h"

namespace dgae {

constexpr int WAVES = 4;                      // wavefronts per workgroup of the narrow kernel
constexpr int MAX_BLOCKS = 2048;              // 256 CUs x 8 workgroups of 4 wavefronts: every SIMD full; beyond, the kernels stride over the envs

struct Params {
    const float *reward, *vf, *last_vf;
    const uint16_t *uid, *uid_next;
    const uint8_t *end;
    float *adv, *target;
    uint8_t *live;
    int32_t T, E, U, scan;                    // scan: slots behind its own a lane looks at (0 ... U - 1)
    float gamma, lambda;
};

// what a lane reads of row (t, e, s)
struct Row {
    uint32_t w, wn;
    float rw, v;
};

__device__ __forceinline__ Row load_row(const Params &g, bool active, size_t i)
{
    Row r{0u, 0u, 0.f, 0.f};
    if (active) { r.w = g.uid[i]; r.wn = g.uid_next[i]; r.rw = g.reward[i]; r.v = g.vf[i]; }
    return r;
}

// One row's step: (r, nv, A) are the reward and the carry at the slot where the word was found.  Writes the three outputs and leaves the
// carry of this slot in (nv, A).
__device__ __forceinline__ void finish_row(const Params &g, bool active, bool found, size_t i, float v, float r, float gl, float &nv, float &A)
{
    // every operation rounded on its own, as in gae_kernel: plain operators under this pragma
#pragma clang fp contract(off)
    const float d = (r + g.gamma * nv) - v;
    const float a = d + gl * A;
    const float tgt = a + v;
    A = found ? a : 0.f;
    nv = found ? v : 0.f;
    if (active) {
        g.adv[i] = A;
        g.target[i] = found ? tgt : 0.f;
        g.live[i] = found ? 1 : 0;
    }
}

template <int UPAD>
__global__ __launch_bounds__(WAVES * 64) void gae_uid_wave_kernel(const Params g)
{
#pragma clang fp contract(off)
    constexpr int GPW = 64 / UPAD;            // envs per wavefront
    const int lane = threadIdx.x & 63, u = lane % UPAD;
    const int64_t wave = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * WAVES;
    const float gl = g.gamma * g.lambda;
    const size_t step = (size_t)g.E * (size_t)g.U;
    for (int64_t first = wave * GPW; first < g.E; first += waves * GPW) {          // uniform in the wavefront
        const int64_t env = first + lane / UPAD;
        const bool active = env < g.E && u < g.U;
        const size_t col = active ? (size_t)env * (size_t)g.U + (size_t)u : 0;
        float nv = (active && g.last_vf) ? g.last_vf[col] : 0.f, A = 0.f;
        Row next = load_row(g, active, (size_t)(g.T - 1) * step + col);
        for (int t = g.T - 1; t >= 0; t--) {
            const size_t i = (size_t)t * step + col;
            const Row row = next;
            if (t > 0) next = load_row(g, active, i - step);                       // in flight while this step computes
            if (g.end && g.end[t]) { nv = 0.f; A = 0.f; }
            int sp = u;
            bool found = false;
            for (int k = 0; k <= g.scan; k++) {                                    // uniform: every lane takes part in every shuffle
                const int s = u - k;
                const uint32_t there = __shfl(row.wn, s > 0 ? s : 0, UPAD);
                if (!found && s >= 0 && there == row.w) { found = true; sp = s; }
            }
            found = found && row.w != 0u;
            const float r = __shfl(row.rw, sp, UPAD), cnv = __shfl(nv, sp, UPAD), cA = __shfl(A, sp, UPAD);
            nv = cnv; A = cA;
            finish_row(g, active, found, i, row.v, r, gl, nv, A);
        }
    }
}

__global__ __launch_bounds__(DCOMP_MAX_UE) void gae_uid_block_kernel(const Params g)
{
#pragma clang fp contract(off)
    __shared__ uint16_t s_wn[DCOMP_MAX_UE];
    __shared__ float s_rw[DCOMP_MAX_UE], s_nv[DCOMP_MAX_UE], s_A[DCOMP_MAX_UE];
    const int u = threadIdx.x;                                                     // blockDim.x = U rounded up to whole wavefronts
    const bool active = u < g.U;
    const float gl = g.gamma * g.lambda;
    const size_t step = (size_t)g.E * (size_t)g.U;
    for (int64_t env = blockIdx.x; env < g.E; env += gridDim.x) {                  // uniform in the workgroup
        const size_t col = active ? (size_t)env * (size_t)g.U + (size_t)u : 0;
        float nv = (active && g.last_vf) ? g.last_vf[col] : 0.f, A = 0.f;
        Row next = load_row(g, active, (size_t)(g.T - 1) * step + col);
        for (int t = g.T - 1; t >= 0; t--) {
            const size_t i = (size_t)t * step + col;
            const Row row = next;
            if (t > 0) next = load_row(g, active, i - step);
            if (g.end && g.end[t]) { nv = 0.f; A = 0.f; }
            s_wn[u] = (uint16_t)row.wn; s_rw[u] = row.rw; s_nv[u] = nv; s_A[u] = A;
            __syncthreads();
            int sp = u;
            bool found = false;
            if (row.w != 0u) {
                const int lo = u - g.scan > 0 ? u - g.scan : 0;
                for (int s = u; s >= lo; s--)
                    if (s_wn[s] == row.w) { found = true; sp = s; break; }
            }
            const float r = s_rw[sp];
            nv = s_nv[sp]; A = s_A[sp];
            __syncthreads();                                                       // everyone has read before the next step publishes
            finish_row(g, active, found, i, row.v, r, gl, nv, A);
        }
    }
}

typedef void (*kernel_fn)(const Params);
static kernel_fn pick_wave_kernel(int U, int *gpw)
{
    int upad = 1;
    while (upad < U) upad *= 2;
    *gpw = 64 / upad;
    switch (upad) {
    case 1: return gae_uid_wave_kernel<1>;
    case 2: return gae_uid_wave_kernel<2>;
    case 4: return gae_uid_wave_kernel<4>;
    case 8: return gae_uid_wave_kernel<8>;
    case 16: return gae_uid_wave_kernel<16>;
    case 32: return gae_uid_wave_kernel<32>;
    default: return gae_uid_wave_kernel<64>;
    }
}

}  // namespace dgae

extern "C" int dcomp_gae_uid(const dcomp_gae_uid_args *g, void *stream)
{
    using namespace dgae;
    if (!g) return fail(DCOMP_EINVAL, "dcomp_gae_uid: args must not be NULL");
    if (int rc = check_struct("dcomp_gae_uid", "dcomp_gae_uid_args", g->struct_size, sizeof(dcomp_gae_uid_args))) return rc;
    if (!g->reward || !g->vf || !g->uid || !g->uid_next || !g->advantages || !g->value_targets || !g->live)
        return fail(DCOMP_EINVAL, "dcomp_gae_uid: reward, vf, uid, uid_next, advantages, value_targets and live must not be NULL");
    if (g->num_steps < 1) return fail(DCOMP_EINVAL, "dcomp_gae_uid: num_steps %d < 1", g->num_steps);
    if (g->num_envs < 1) return fail(DCOMP_EINVAL, "dcomp_gae_uid: num_envs %d < 1", g->num_envs);
    if (g->num_slots < 1 || g->num_slots > DCOMP_MAX_UE) return fail(DCOMP_EINVAL, "dcomp_gae_uid: num_slots %d outside 1 ... %d", g->num_slots, DCOMP_MAX_UE);
    if ((int64_t)g->num_steps * g->num_envs * g->num_slots >= (1ll << 40))
        return fail(DCOMP_EINVAL, "dcomp_gae_uid: num_steps x num_envs x num_slots = %d x %d x %d is 2^40 elements or more", g->num_steps, g->num_envs, g->num_slots);
    Params k;
    k.reward = g->reward; k.vf = g->vf; k.last_vf = g->last_vf; k.uid = g->uid; k.uid_next = g->uid_next; k.end = g->end;
    k.adv = g->advantages; k.target = g->value_targets; k.live = g->live;
    k.T = g->num_steps; k.E = g->num_envs; k.U = g->num_slots; k.gamma = g->gamma; k.lambda = g->lambda;
    k.scan = (g->max_shift < 0 || g->max_shift > g->num_slots - 1) ? g->num_slots - 1 : g->max_shift;
    if (g->num_slots <= 64) {
        int gpw = 1;
        const kernel_fn fn = pick_wave_kernel(g->num_slots, &gpw);
        const int64_t want = ((int64_t)g->num_envs + (int64_t)gpw * WAVES - 1) / ((int64_t)gpw * WAVES);
        hipLaunchKernelGGL(fn, dim3((unsigned)(want < MAX_BLOCKS ? want : MAX_BLOCKS)), dim3(WAVES * 64), 0, static_cast<hipStream_t>(stream), k);
    } else {
        const int grid = g->num_envs < MAX_BLOCKS ? g->num_envs : MAX_BLOCKS;
        hipLaunchKernelGGL(gae_uid_block_kernel, dim3(grid), dim3((g->num_slots + 63) / 64 * 64), 0, static_cast<hipStream_t>(stream), k);
    }
    HIP_TRY(hipGetLastError());
    return DCOMP_OK;
}
