// dcomp_learner.hip -- the PPO learner of the fcnet a dcomp_actor runs (include/dcomp_learner.h): loss, backward pass and Adam; and
// its minibatches picked through a row index out of a whole sample batch, rows or compact record (include/dcomp_learner_indexed.h);
// and the learners of a per-UE policy set trained in one launch round (include/dcomp_learner_group.h): the same four kernels with the
// policy as a grid dimension, behind the per-learner ones below; and the gradients as a running sum the caller owns, for micro-batches
// and data-parallel ranks (include/dcomp_learner_accum.h): accumulate_kernel in reduce_kernel's place, then norm_kernel / finish_kernel;
// and those three with the policy as a grid dimension, for the accumulators of a whole group (include/dcomp_learner_group_accum.h).
// The bodies the per-learner and grouped forms share are text (dcomp_learner_tiles.inc, dcomp_learner_reduce.inc,
// dcomp_learner_adam.inc, dcomp_learner_accumulate.inc, dcomp_learner_norm.inc, dcomp_learner_finish.inc), included in each kernel.
//
// Four kernels per minibatch, all deterministic (no floating-point atomics; every sum has an order fixed by the row count):
//   learner_kernel   forward + loss + backward-data.  The shape of actor_kernel: a wavefront owns 32 decision rows on its lanes and
//                    runs layers 1-3 transposed on v_mfma_f32_32x32x16_bf16, the logits pass through the [32][33] LDS tile and lane r
//                    walks row r's columns -- with the GIVEN action.  Layer 1, the hidden fragments, the logit tile and the online
//                    log-sum-exp step are the actor's own functions (dcomp_actor_impl.h), so at unchanged weights logp is what the
//                    actor wrote, bit for bit; the weights of layers 2 and 3 stream group by group here (tile_dot), not through the
//                    actor's ring: one wave per SIMD has the registers for whole groups.  A second walk over the recomputed logits
//                    writes dlogits back into the tile.  Backward stays transposed: dH2^T = W3 dlogits^T, dH1^T = W2 dA2^T with the weights as the A
//                    operand in the OTHER orientation (a second packed copy, w2b / w3b); the accumulator has the hidden unit in its
//                    register and the row on its lane exactly like the h fragments, so (.) act'(h) and the bf16 conversion stay in
//                    registers.  The value trunk is a second sweep.  x, h1, h2, dA1, dA2, dlogits go to HBM as bf16 [width][rows]
//                    (64-byte runs per store instruction) for the weight gradients; per-tile sums of the statistics to a workspace.
//   wgrad_kernel     dW[in][out] = sum over rows a (x) d: rows are the K axis here, and in [width][rows] order both MFMA operands are
//                    one 16-byte load per lane.  One wave per (block of up to 2 x 4 tiles of 32 x 32, row chunk): six operand loads
//                    feed eight MFMAs; f32 partials per chunk; the bias gradient is one more MFMA against a fragment of ones.
//   reduce_kernel    sums the chunk partials in chunk order, applies 1 / N once, writes the natural [in][out] gradients; and the
//                    five statistics from the per-tile sums.
//   adam_kernel      adam_reference (deepcomp_amd/learner.py) under `#pragma clang fp contract(off)`, then each thread scatters
//                    its weight as bf16 into the actor handle's packed fragments, in both orientations, where pack_index() (the
//                    function pack() places its elements with) says.
// Padded hidden units: the packed copies hold zeros there, forward (h = act(0) = 0) and backward (a zero row of w3b / w2b gives
// dH = 0), no kernel ever writes a padded entry, and reduce / adam only visit real entries.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#define DCOMP_BUILDING_LIBRARY 1
#include "../../include/dcomp.h"
#include "../../include/dcomp_learner.h"
#include "../../include/dcomp_learner_indexed.h"
#include "../../include/dcomp_learner_group.h"
#include "../../include/dcomp_learner_accum.h"
#include "../../include/dcomp_learner_group_accum.h"
#include "dcomp_actor_impl.h"       // the forward-pass helpers, the fragment layout, Net and struct dcomp_actor, fail / HIP_TRY: shared with dcomp_actor.hip

namespace dlearn {

using namespace dactor;

// the kernels' names for the plan's constants (dcomp_fcnet_plan.h): equal, or this does not compile
constexpr int CHUNK_UNIT = 2048;          // rows of a weight-gradient chunk: CHUNK_UNIT x the smallest factor that keeps ...
constexpr int MAX_CHUNKS = 128;           // ... the chunk count at or below this
static_assert(CHUNK_UNIT == dplan::CHUNK_UNIT && MAX_CHUNKS == dplan::MAX_CHUNKS, "dcomp_fcnet_plan.h plans for other constants");

struct LParams {
    const float *obs;
    const uint8_t *actions;
    const float *old_logp, *old_logits, *adv, *vtarg, *old_vf;
    float *o_logp, *o_ent, *o_kl, *o_vf, *o_ratio;
    const float *up_dlogits, *up_dvalue;
    Net net;                                          // the actor handle's: its forward fragments are the learner's
    const uint4 *w2b, *w3b, *vw2b, *vw3b;             // the backward orientation
    __bf16 *X, *H1, *H2, *D1, *D2, *D3, *VH1, *VH2, *VD1, *VD2, *VD3;    // [width][ld]
    float4 *headws;                                   // [rows][heads]: lse, old lse, entropy of the head
    double *part;                                     // [tiles][4]: sums of surrogate, kl, entropy, vf loss over the tile's counted rows
    int64_t rows, tiles, ld;
    int32_t num_active, fwd_only, upstream;
    float clip, vf_clip, vf_coeff, ent_coeff, kl_coeff;
};
// the arguments of the indexed instantiations (dcomp_learner_indexed.h): position i of the minibatch reads source row index[i]
// (NULL: i) of a sample batch of source_rows rows; compact: obs is the record of source_rows / U envs
struct IParams : LParams {
    const int32_t *index;
    int64_t source_rows;
    int32_t compact;
};

constexpr uint32_t NO_ROW = 0xFFFFFFFFu;  // ri of a position that reads nothing (a valid source row is < 2^31)

// one output tile of a hidden -> out layer: sum over the 2 MT k steps of fragments first ... of w with the B fragments b
template <int MT> __device__ __forceinline__ f32x16 tile_dot(const uint4 *w, size_t first, const bf16x8 (&b)[MT][2], uint32_t lane16)
{
    constexpr int KS2 = 2 * MT, D = KS2 < 8 ? KS2 : 8;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.f;
#pragma unroll
    for (int g = 0; g < KS2; g += D) {
        uint4 q[D];
#pragma unroll
        for (int i = 0; i < D; i++) q[i] = load_frag(w, first + g + i, lane16);
#pragma unroll
        for (int i = 0; i < D; i++) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(q[i]), b[(g + i) >> 1][(g + i) & 1], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);               // (group by group: left alone every load of the layer is hoisted to its top)
    }
    return acc;
}

// the fragments of a layer's activations or deltas -> ws[unit][ld] at column col: element j of f[t][s] on lane half h is unit
// 32 t + 16 s + 8 (j >> 2) + 4 h + (j & 3); the 32 lanes of a half write one 64-byte run per element
template <int MT> __device__ __forceinline__ void store_frags(__bf16 *ws, int64_t ld, uint32_t voff, const bf16x8 (&f)[MT][2])
{
    // voff = the lane's byte offset 2 (column + 4 h ld) (< 2^32: dcomp_learner_create bounds max_rows); the unit's part of the address is
    // uniform.  Opaque at every store, as in load_frag: hoisted out of the tile loop the ~600 lane addresses would be spilled registers.
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                asm volatile("" : "+v"(voff));
                char *row = reinterpret_cast<char *>(ws) + (size_t)(32 * t + 16 * s + 8 * (j >> 2) + (j & 3)) * (size_t)ld * 2;
                *reinterpret_cast<__bf16 *>(row + voff) = f[t][s][j];
            }
}

// d = bf16(dH (.) act'(h)), h the stored bf16 activation
template <int MT, bool RELU> __device__ __forceinline__ void delta_frags(const f32x16 (&dh)[MT], const bf16x8 (&hf)[MT][2], bf16x8 (&d)[MT][2])
{
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float hv = (float)hf[t][s][j], g = dh[t][8 * s + j];
                d[t][s][j] = (__bf16)(RELU ? (hv > 0.f ? g : 0.f) : g * (1.f - hv * hv));
            }
}

// the source row of the position on this lane: IDX, what the tile's resolve step left in ri (read from LDS at every use: not a
// register held across the sweeps); otherwise the position itself
template <bool IDX> __device__ __forceinline__ size_t source_row(const uint32_t *ri, int r, int64_t myrow)
{
    return IDX ? (size_t)ri[r * 4] : (size_t)myrow;
}

// a fixed tree over the 64 lanes.  In double: the statistics are means of f32 row terms summed in double (reduce_kernel), and an f32
// tree here would put its own rounding (a few 2^-24 of the tile's sum) into a mean that is otherwise exact up to its last rounding --
// with few rows that is the statistic's last bit
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// IDX: the per-row inputs come from source row index[i] of the whole sample batch, as rows or as the compact record (the indexed
// entry points); the workspaces, the partials and the per-row outputs stay at minibatch position i.  A template parameter: the
// instantiations without it are the kernel as it was.
template <int MT, bool RELU, bool IDX>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void learner_kernel(const std::conditional_t<IDX, IParams, LParams> p)
{
#include "dcomp_learner_tiles.inc"
}

typedef void (*learner_fn)(const LParams);
typedef void (*indexed_fn)(const IParams);
static learner_fn pick(int mt, bool relu)
{
    return pick_shape(mt, relu, [](auto s) -> learner_fn { return learner_kernel<decltype(s)::MT, decltype(s)::RELU, false>; });
}
static indexed_fn pick_indexed(int mt, bool relu)
{
    return pick_shape(mt, relu, [](auto s) -> indexed_fn { return learner_kernel<decltype(s)::MT, decltype(s)::RELU, true>; });
}

// ---------------------------------------------------------------- weight gradients
struct WDesc {
    const __bf16 *a, *d;                  // [in_p][ld], [out_p][ld]
    float *part, *bpart;                  // [chunk][in_p][out_p], [chunk][out_p]
    int32_t mi_tiles, ni_tiles, first_task, nmain;     // nmain block tasks, then ni_tiles / NB bias tasks
};
struct WParams {
    WDesc g[6];
    int64_t ld, rows_pad, chunk_rows;
    int32_t ntask;
};

// a wave's block of dW: MB x NB tiles of 32 x 32, wgrad_mb x wgrad_nb of the product's tile counts (dcomp_fcnet_plan.h)
template <int MB, int NB>
__device__ __forceinline__ void wgrad_block(const WParams &p, const WDesc &g, int local, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    const int nblk = g.ni_tiles / NB, mi0 = (local / nblk) * MB, ni0 = (local % nblk) * NB;
    const int64_t chunk = blockIdx.y, k0 = chunk * p.chunk_rows;
    const int64_t k1 = k0 + p.chunk_rows < p.rows_pad ? k0 + p.chunk_rows : p.rows_pad;
    const __bf16 *ap = g.a + (size_t)(32 * mi0 + r) * (size_t)p.ld + 8 * h;
    const __bf16 *dp = g.d + (size_t)(32 * ni0 + r) * (size_t)p.ld + 8 * h;
    const size_t tile_stride = (size_t)32 * (size_t)p.ld;
    f32x16 acc[MB][NB];
#pragma unroll
    for (int j = 0; j < NB; j++)
#pragma unroll
        for (int e = 0; e < 16; e++)
#pragma unroll
            for (int i = 0; i < MB; i++) acc[i][j][e] = 0.f;
    for (int64_t k = k0; k < k1; k += 16) {
        bf16x8 A[MB], B[NB];
#pragma unroll
        for (int i = 0; i < MB; i++) A[i] = as_frag(*reinterpret_cast<const uint4 *>(ap + i * tile_stride + k));
#pragma unroll
        for (int j = 0; j < NB; j++) B[j] = as_frag(*reinterpret_cast<const uint4 *>(dp + j * tile_stride + k));
#pragma unroll
        for (int j = 0; j < NB; j++)
#pragma unroll
            for (int i = 0; i < MB; i++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[i], B[j], acc[i][j], 0, 0, 0);
    }
    const int in_p = 32 * g.mi_tiles, out_p = 32 * g.ni_tiles;
    float *dst = g.part + (size_t)chunk * (size_t)in_p * out_p;
#pragma unroll
    for (int i = 0; i < MB; i++)
#pragma unroll
        for (int j = 0; j < NB; j++)
#pragma unroll
            for (int e = 0; e < 16; e++)
                dst[(size_t)(32 * (mi0 + i) + (e & 3) + 8 * (e >> 2) + 4 * h) * out_p + 32 * (ni0 + j) + r] = acc[i][j][e];
}

// the bias gradients of NB output tiles: the column sums of d as one MFMA per tile against a fragment of ones (every row of the
// product holds them; row 0 is stored)
template <int NB>
__device__ __forceinline__ void wgrad_bias(const WParams &p, const WDesc &g, int blk, int lane)
{
    const int r = lane & 31, h = lane >> 5, ni0 = blk * NB;
    const int64_t chunk = blockIdx.y, k0 = chunk * p.chunk_rows;
    const int64_t k1 = k0 + p.chunk_rows < p.rows_pad ? k0 + p.chunk_rows : p.rows_pad;
    const __bf16 *dp = g.d + (size_t)(32 * ni0 + r) * (size_t)p.ld + 8 * h;
    const size_t tile_stride = (size_t)32 * (size_t)p.ld;
    f32x16 bacc[NB];
#pragma unroll
    for (int j = 0; j < NB; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) bacc[j][e] = 0.f;
    bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; j++) ones[j] = (__bf16)1.f;
    for (int64_t k = k0; k < k1; k += 16) {
#pragma unroll
        for (int j = 0; j < NB; j++)
            bacc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, as_frag(*reinterpret_cast<const uint4 *>(dp + j * tile_stride + k)), bacc[j], 0, 0, 0);
    }
    if (h == 0) {
#pragma unroll
        for (int j = 0; j < NB; j++) g.bpart[(size_t)chunk * 32 * g.ni_tiles + 32 * (ni0 + j) + r] = bacc[j][0];
    }
}

__global__ __launch_bounds__(BLOCK) void wgrad_kernel(const WParams p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int task = blockIdx.x * WAVES + wave;
    if (task >= p.ntask) return;
    int gi = 0;
#pragma unroll
    for (int i = 1; i < 6; i++) gi = task >= p.g[i].first_task ? i : gi;
    const WDesc g = p.g[gi];
    const int local = task - g.first_task, mb = wgrad_mb(g.mi_tiles), nb = wgrad_nb(g.ni_tiles);      // (wave-uniform)
    if (local >= g.nmain) {                                                           // behind a product's blocks: its bias tasks
        if (nb == 4) wgrad_bias<4>(p, g, local - g.nmain, lane);
        else wgrad_bias<1>(p, g, local - g.nmain, lane);
    } else if (mb == 2 && nb == 4) wgrad_block<2, 4>(p, g, local, lane);
    else if (nb == 4) wgrad_block<1, 4>(p, g, local, lane);
    else if (mb == 2) wgrad_block<2, 1>(p, g, local, lane);
    else wgrad_block<1, 1>(p, g, local, lane);
}

// ---------------------------------------------------------------- the natural-layout arrays
struct ADesc {
    int32_t off, nin, nout, out_p, in_p, is_bias;            // [nin][nout] at `off` of the flat arrays (a bias: nin = 1)
    const float *part;                                       // chunk partials ([chunk][in_p][out_p] / [chunk][out_p])
    // repack targets: a weight goes as bf16 into the forward fragments and, layers 2 and 3, the backward ones; a bias as f32
    uint16_t *fwd, *bwd;
    float *bias;
    int32_t fwd_ks, fwd_perm, bwd_ks, bwd_perm;
};
struct AParams {
    ADesc a[NARR];
    int32_t total, nchunks;
    float scale;
    float *w, *g, *m, *v;
    const double *tile_part;                                 // [tiles][4]
    int64_t tiles;
    float *stats;
    double count;
    float vf_coeff, ent_coeff, kl_coeff;
    int32_t adam, want_stats;
    float beta1, omb1, beta2, omb2, step_size, bc2_sqrt, eps;
};

template <class P> __device__ __forceinline__ int find_array(const P &p, int e)      // (P: AParams, or the grouped kernels' view of it)
{
    int ai = 0;
#pragma unroll
    for (int i = 1; i < NARR; i++) ai = e >= p.a[i].off ? i : ai;
    return ai;
}

__global__ __launch_bounds__(256) void reduce_kernel(const AParams p)
{
#include "dcomp_learner_reduce.inc"
}

__global__ __launch_bounds__(256) void adam_kernel(const AParams p)
{
#include "dcomp_learner_adam.inc"
}

// ---------------------------------------------------------------- accumulated gradients (include/dcomp_learner_accum.h)
// reduce_kernel's loop with the running sum carried in: acc += the chunk partials in chunk order, unscaled; the four loss sums of the
// per-tile workspace (reduce_kernel's 256 ranges, then the 256 sums in order) and the counted rows are added to sums.  One launch per
// (micro-)batch on one stream: a thread owns its entry of acc, thread 0 of block 0 owns sums -- no atomics.
__global__ __launch_bounds__(256) void accumulate_kernel(const AParams p, float *acc, double *sums)
{
#include "dcomp_learner_accumulate.inc"
}

struct FParams {
    const float *acc;                                        // [total]
    const double *sums;                                      // [DCOMP_ACCUM_SUMS]
    float *g, *stats, *grad_norm;                            // the handle's gradients; stats and grad_norm may be NULL
    double *norm_part;                                       // [nparts]: the handle's workspace
    int32_t total, nparts, want_norm;
    float clip, vf_coeff, ent_coeff, kl_coeff;
};
constexpr int NORM_SPAN = 4096;                              // entries of a norm_kernel block: 16 per thread

// 1 / N from the accumulated count, as learner_launch forms reduce_kernel's scale on the host
__device__ __forceinline__ float accum_scale(const double *sums) { return sums[4] > 0. ? (float)(1.0 / sums[4]) : 0.f; }

// the squares of the scaled gradients, in double: a thread its 16 entries in order, a fixed tree over the block, one partial per block
__global__ __launch_bounds__(256) void norm_kernel(const FParams p)
{
#include "dcomp_learner_norm.inc"
}

// g = acc / N (x the clip coefficient), and the statistics from sums as reduce_kernel forms them from its totals.  Every block adds
// the norm partials itself, in block order: the same number in every block.
__global__ __launch_bounds__(256) void finish_kernel(const FParams p)
{
#include "dcomp_learner_finish.inc"
}

// ---------------------------------------------------------------- all learners of a group in one launch (include/dcomp_learner_group.h)
// The four kernels above with the policy as a grid dimension.  What dcomp_learner keeps in lp / wp / ap is one entry per policy of a
// device table written at dcomp_learner_group_create; what changes per call (rows, hyper-parameters, Adam's scalars) are arrays in
// the kernel arguments, indexed like the table by the policy's number within the launch's slice.  The policy is wave-uniform
// (blockIdx), so read through the constant address space an entry arrives in SGPRs like the kernel arguments it stands for
// (actor_kernel<..., PER = true> reads its trunk table the same way), and every statement of a policy's arithmetic is the
// per-learner kernel's own (the .inc bodies).
constexpr int GROUP_SLICE = DCOMP_GROUP_SLICE;

struct GEntry {
    LParams lp;                           // first: the member's net, backward fragments, workspaces and ld (the per-call members unused)
    WDesc wg[6];
    ADesc a[NARR];
    float *w, *g, *m, *v;
    int32_t total, ntask;
    float beta1, omb1, beta2, omb2, eps;
    int32_t reserved;
    double *norm_part;                    // appended (the offsets above stay put): the member's norm workspace, for finish_group_kernel
    int32_t norm_parts, reserved2;
};
typedef const GEntry __attribute__((address_space(4))) *gentry_ptr;
__device__ __forceinline__ gentry_ptr group_entry(const GEntry *table, int i) { return (gentry_ptr)(uintptr_t)(table + i); }
// a whole member of an entry through the constant address space, as 64-bit words (slot_trunk's way, dcomp_actor.hip)
template <class T> __device__ __forceinline__ T const_copy(const T __attribute__((address_space(4))) *src)
{
    static_assert(sizeof(T) % 8 == 0 && std::is_trivially_copyable<T>::value, "read as 64-bit words");
    const uint64_t __attribute__((address_space(4))) *q = (const uint64_t __attribute__((address_space(4))) *)src;
    union { T v; uint64_t w[sizeof(T) / 8]; } u;
#pragma unroll
    for (size_t i = 0; i < sizeof(T) / 8; i++) u.w[i] = q[i];
    return u.v;
}

// learner_kernel<MT, RELU, true> per policy.  The members a grouped call never uses (per-row outputs, upstream gradients, fwd_only)
// are arguments all the same, NULL / 0 from the host: known at compile time they would prune the body, and which f32 operations
// the compiler contracts must not depend on who launches it.
struct GLParams {
    const float *obs;
    const uint8_t *actions;
    const float *old_logp, *old_logits, *adv, *vtarg, *old_vf;
    float *o_logp, *o_ent, *o_kl, *o_vf, *o_ratio;
    const float *up_dlogits, *up_dvalue;
    const GEntry *table;                  // of the slice's first policy, as index is
    const int32_t *index;
    int64_t index_stride, source_rows;
    int32_t compact, num_active, fwd_only, upstream;
    int32_t rows[GROUP_SLICE];            // 0: the policy sits this call out
    float clip[GROUP_SLICE], vf_clip[GROUP_SLICE], vf_coeff[GROUP_SLICE], ent_coeff[GROUP_SLICE], kl_coeff[GROUP_SLICE];
};

template <int MT, bool RELU>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void learner_group_kernel(const GLParams gp)
{
    constexpr bool IDX = true;
    const int pol = blockIdx.y;
    const int32_t nrows = gp.rows[pol];
    if (nrows == 0 || (int64_t)blockIdx.x * WAVES >= tiles_of(nrows)) return;        // not in this call; beyond the policy's tiles
    IParams p;
    static_cast<LParams &>(p) = const_copy(&group_entry(gp.table, pol)->lp);
    p.obs = gp.obs; p.actions = gp.actions; p.old_logp = gp.old_logp; p.old_logits = gp.old_logits; p.adv = gp.adv; p.vtarg = gp.vtarg; p.old_vf = gp.old_vf;
    p.o_logp = gp.o_logp; p.o_ent = gp.o_ent; p.o_kl = gp.o_kl; p.o_vf = gp.o_vf; p.o_ratio = gp.o_ratio;
    p.up_dlogits = gp.up_dlogits; p.up_dvalue = gp.up_dvalue;
    p.rows = nrows; p.tiles = tiles_of(nrows);
    p.num_active = gp.num_active; p.fwd_only = gp.fwd_only; p.upstream = gp.upstream;
    p.clip = gp.clip[pol]; p.vf_clip = gp.vf_clip[pol]; p.vf_coeff = gp.vf_coeff[pol]; p.ent_coeff = gp.ent_coeff[pol]; p.kl_coeff = gp.kl_coeff[pol];
    p.index = gp.index + (int64_t)pol * gp.index_stride; p.source_rows = gp.source_rows; p.compact = gp.compact;
    {
#include "dcomp_learner_tiles.inc"
    }
}

typedef void (*group_fn)(const GLParams);
static group_fn pick_group(int mt, bool relu)
{
    return pick_shape(mt, relu, [](auto s) -> group_fn { return learner_group_kernel<decltype(s)::MT, decltype(s)::RELU>; });
}

// wgrad_kernel per policy (blockIdx.z), the row split from the policy's own row count
struct GWParams {
    const GEntry *table;
    int32_t rows[GROUP_SLICE];
};

__global__ __launch_bounds__(BLOCK) void wgrad_group_kernel(const GWParams gp)
{
    const int pol = blockIdx.z;
    const int32_t nrows = gp.rows[pol];
    if (nrows == 0) return;
    const RowSplit rs = row_split(nrows);
    if ((int)blockIdx.y >= rs.nchunks) return;                                        // beyond the policy's chunks
    const gentry_ptr en = group_entry(gp.table, pol);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int task = blockIdx.x * WAVES + wave;
    if (task >= en->ntask) return;
    int gi = 0;
#pragma unroll
    for (int i = 1; i < 6; i++) gi = task >= en->wg[i].first_task ? i : gi;
    const WDesc g = const_copy(&en->wg[gi]);
    WParams p;                                                                        // (what wgrad_block / wgrad_bias read of it)
    p.ld = en->lp.ld; p.rows_pad = rs.rows_pad; p.chunk_rows = rs.chunk_rows;
    const int local = task - g.first_task, mb = wgrad_mb(g.mi_tiles), nb = wgrad_nb(g.ni_tiles);      // (wave-uniform)
    if (local >= g.nmain) {
        if (nb == 4) wgrad_bias<4>(p, g, local - g.nmain, lane);
        else wgrad_bias<1>(p, g, local - g.nmain, lane);
    } else if (mb == 2 && nb == 4) wgrad_block<2, 4>(p, g, local, lane);
    else if (nb == 4) wgrad_block<1, 4>(p, g, local, lane);
    else if (mb == 2) wgrad_block<2, 1>(p, g, local, lane);
    else wgrad_block<1, 1>(p, g, local, lane);
}

// a policy's AParams as reduce_kernel / adam_kernel name them: the array descriptions stay in the table (a thread's own is a
// divergent index; the offsets find_array compares are at uniform addresses and compile to scalar loads as they are:
// adam_group_kernel has adam_kernel's 16 vector-memory instructions), everything else is scalar
struct GAView {
    const ADesc *a;
    int32_t total, nchunks;
    float scale;
    float *w, *g, *m, *v;
    const double *tile_part;
    int64_t tiles;
    float *stats;
    double count;
    float vf_coeff, ent_coeff, kl_coeff;
    int32_t adam, want_stats;
    float beta1, omb1, beta2, omb2, step_size, bc2_sqrt, eps;
};
__device__ __forceinline__ GAView group_view(const GEntry *table, int pol)
{
    const gentry_ptr en = group_entry(table, pol);
    GAView p = {};
    p.a = table[pol].a;
    p.total = en->total; p.w = en->w; p.g = en->g; p.m = en->m; p.v = en->v; p.tile_part = en->lp.part;
    return p;
}

// reduce_kernel per policy (blockIdx.y): 1 / N from the host as launch computes it, the count and the split from the row count
struct GRParams {
    const GEntry *table;
    float *stats;                         // [policy of the slice][DCOMP_PPO_NUM_STATS]
    int32_t rows[GROUP_SLICE];
    float scale[GROUP_SLICE], vf_coeff[GROUP_SLICE], ent_coeff[GROUP_SLICE], kl_coeff[GROUP_SLICE];
};

__global__ __launch_bounds__(256) void reduce_group_kernel(const GRParams gp)
{
    const int pol = blockIdx.y;
    const int32_t nrows = gp.rows[pol];
    if (nrows == 0) return;
    GAView p = group_view(gp.table, pol);
    const RowSplit rs = row_split(nrows);
    p.nchunks = rs.nchunks; p.tiles = rs.tiles; p.scale = gp.scale[pol]; p.count = (double)nrows;
    p.stats = gp.stats + DCOMP_PPO_NUM_STATS * pol; p.want_stats = 1;
    p.vf_coeff = gp.vf_coeff[pol]; p.ent_coeff = gp.ent_coeff[pol]; p.kl_coeff = gp.kl_coeff[pol];
    {
#include "dcomp_learner_reduce.inc"
    }
}

// adam_kernel per policy (blockIdx.y): the bias corrections per policy from the host, in double as launch_adam has them -- the
// members have taken different numbers of steps
struct GAParams {
    const GEntry *table;
    int32_t active[GROUP_SLICE];
    float step_size[GROUP_SLICE], bc2_sqrt[GROUP_SLICE];
};

__global__ __launch_bounds__(256) void adam_group_kernel(const GAParams gp)
{
    const int pol = blockIdx.y;
    if (!gp.active[pol]) return;
    GAView p = group_view(gp.table, pol);
    const gentry_ptr en = group_entry(gp.table, pol);
    p.adam = 1; p.beta1 = en->beta1; p.omb1 = en->omb1; p.beta2 = en->beta2; p.omb2 = en->omb2; p.eps = en->eps;
    p.step_size = gp.step_size[pol]; p.bc2_sqrt = gp.bc2_sqrt[pol];
    {
#include "dcomp_learner_adam.inc"
    }
}

// accumulate_kernel per policy (blockIdx.y) on the policy's slices of the caller's [P][flat] / [P][DCOMP_ACCUM_SUMS] accumulators: the
// split and the count from the row count, as reduce_group_kernel has them
struct GCParams {
    const GEntry *table;
    float *acc;                           // of the slice's first policy, as table is
    double *sums;
    int32_t rows[GROUP_SLICE];            // 0: the policy sits this call out, its slices are not touched
};

__global__ __launch_bounds__(256) void accumulate_group_kernel(const GCParams gp)
{
    const int pol = blockIdx.y;
    const int32_t nrows = gp.rows[pol];
    if (nrows == 0) return;
    GAView p = group_view(gp.table, pol);
    const RowSplit rs = row_split(nrows);
    p.nchunks = rs.nchunks; p.tiles = rs.tiles; p.count = (double)nrows;
    float *acc = gp.acc + (size_t)pol * (size_t)p.total;
    double *sums = gp.sums + DCOMP_ACCUM_SUMS * pol;
    {
#include "dcomp_learner_accumulate.inc"
    }
}

// norm_kernel / finish_kernel per policy (blockIdx.y): the policy's FParams from its table entry and the per-call arrays
struct GFParams {
    const GEntry *table;
    const float *acc;                     // of the slice's first policy
    const double *sums;
    float *stats, *grad_norm;             // [policy of the slice][DCOMP_PPO_NUM_STATS], [policy of the slice]; may be NULL
    int32_t active[GROUP_SLICE], want_norm[GROUP_SLICE];
    float clip[GROUP_SLICE], vf_coeff[GROUP_SLICE], ent_coeff[GROUP_SLICE], kl_coeff[GROUP_SLICE];
};
__device__ __forceinline__ FParams group_finish_params(const GFParams &gp, int pol)
{
    const gentry_ptr en = group_entry(gp.table, pol);
    FParams p;
    p.total = en->total; p.nparts = en->norm_parts; p.g = en->g; p.norm_part = en->norm_part;
    p.acc = gp.acc + (size_t)pol * (size_t)p.total; p.sums = gp.sums + DCOMP_ACCUM_SUMS * pol;
    p.stats = gp.stats ? gp.stats + DCOMP_PPO_NUM_STATS * pol : nullptr; p.grad_norm = gp.grad_norm ? gp.grad_norm + pol : nullptr;
    p.want_norm = gp.want_norm[pol]; p.clip = gp.clip[pol];
    p.vf_coeff = gp.vf_coeff[pol]; p.ent_coeff = gp.ent_coeff[pol]; p.kl_coeff = gp.kl_coeff[pol];
    return p;
}

__global__ __launch_bounds__(256) void norm_group_kernel(const GFParams gp)
{
    const int pol = blockIdx.y;
    if (!gp.active[pol] || !gp.want_norm[pol]) return;
    const FParams p = group_finish_params(gp, pol);
    {
#include "dcomp_learner_norm.inc"
    }
}

__global__ __launch_bounds__(256) void finish_group_kernel(const GFParams gp)
{
    const int pol = blockIdx.y;
    if (!gp.active[pol]) return;
    const FParams p = group_finish_params(gp, pol);
    {
#include "dcomp_learner_finish.inc"
    }
}

static_assert(sizeof(GLParams) <= 4096 && sizeof(GWParams) <= 4096 && sizeof(GRParams) <= 4096 && sizeof(GAParams) <= 4096 &&
              sizeof(GCParams) <= 4096 && sizeof(GFParams) <= 4096,
              "the kernel arguments of a grouped launch: lower DCOMP_GROUP_SLICE");
static_assert(DCOMP_GROUP_SLICE >= 64 && DCOMP_GROUP_SLICE <= 65535, "a slice is a grid's y / z extent");

}  // namespace dlearn

struct dcomp_learner {
    dcomp_actor *a;
    int64_t max_rows, ld, step;
    int32_t device;
    float beta1, beta2, eps;
    void *mem;
    float *w, *g, *m, *v;
    double *norm_part;                    // [norm_parts]: norm_kernel's partials (dcomp_learner_accum_finish)
    int32_t norm_parts;
    dlearn::LearnerPlan plan;             // every shape number of the handle behind the actor's own (a->plan)
    dlearn::LParams lp;                   // the handle's part of the kernel arguments
    dlearn::WParams wp;
    dlearn::AParams ap;
};

static const char *const ARRAY_NAMES[dlearn::NARR] = {"w1", "b1", "w2", "b2", "w3", "b3", "vw1", "vb1", "vw2", "vb2", "wv", "bv"};

static void members(const dcomp_learner_arrays *s, float *(&out)[dlearn::NARR])
{
    float *m[dlearn::NARR] = {s->w1, s->b1, s->w2, s->b2, s->w3, s->b3, s->vw1, s->vb1, s->vw2, s->vb2, s->wv, s->bv};
    for (int i = 0; i < dlearn::NARR; i++) out[i] = m[i];
}

// struct size and, with `all`, every member non-NULL
static int check_arrays(const char *fn, const char *what, const dcomp_learner_arrays *s, bool all)
{
    if (!s) return fail(DCOMP_EINVAL, "%s: %s must not be NULL", fn, what);
    if (int rc = check_struct(fn, "dcomp_learner_arrays", s->struct_size, sizeof(dcomp_learner_arrays))) return rc;
    if (all) {
        float *m[dlearn::NARR];
        members(s, m);
        for (int i = 0; i < dlearn::NARR; i++)
            if (!m[i]) return fail(DCOMP_EINVAL, "%s: %s.%s is NULL", fn, what, ARRAY_NAMES[i]);
    }
    return DCOMP_OK;
}

static void launch_adam(dcomp_learner *l, bool adam, float lr, hipStream_t stream)
{
    dlearn::AParams ap = l->ap;
    ap.adam = adam;
    if (adam) {
        const double t = (double)(l->step + 1);
        ap.beta1 = l->beta1; ap.beta2 = l->beta2; ap.eps = l->eps;
        ap.omb1 = (float)(1.0 - (double)l->beta1); ap.omb2 = (float)(1.0 - (double)l->beta2);
        ap.step_size = (float)((double)lr / (1.0 - std::pow((double)l->beta1, t)));
        ap.bc2_sqrt = (float)std::sqrt(1.0 - std::pow((double)l->beta2, t));
    }
    hipLaunchKernelGGL(dlearn::adam_kernel, dim3((l->plan.total + 255) / 256), dim3(256), 0, stream, ap);
}

extern "C" int dcomp_learner_create(dcomp_actor *a, const dcomp_learner_cfg *cfg, dcomp_learner **out)
{
    using namespace dlearn;
    const char *fn = "dcomp_learner_create";
    if (out) *out = nullptr;
    if (!a || !cfg || !out) return fail(DCOMP_EINVAL, "%s: actor, cfg and out must not be NULL", fn);
    if (int rc = check_struct(fn, "dcomp_learner_cfg", cfg->struct_size, sizeof(dcomp_learner_cfg))) return rc;
    if (cfg->value_shared == 1) return fail(DCOMP_EUNSUPPORTED, "%s: the shared value function (vf_share_layers=True) is not supported: the learner needs a value trunk of its own", fn);
    if (cfg->value_shared != 0) return fail(DCOMP_EINVAL, "%s: value_shared %d is neither 0 nor 1", fn, cfg->value_shared);
    if (cfg->max_rows < 1 || cfg->max_rows > (1ll << 28)) return fail(DCOMP_EINVAL, "%s: max_rows %lld outside [1, 2^28]", fn, (long long)cfg->max_rows);
    if (!(cfg->beta1 >= 0.f && cfg->beta1 < 1.f) || !(cfg->beta2 >= 0.f && cfg->beta2 < 1.f)) return fail(DCOMP_EINVAL, "%s: beta1 %g / beta2 %g outside [0, 1)", fn, cfg->beta1, cfg->beta2);
    if (!(cfg->eps > 0.f)) return fail(DCOMP_EINVAL, "%s: eps %g must be > 0", fn, cfg->eps);
    if (int rc = check_arrays(fn, "cfg.weights", cfg->weights, true)) return rc;
    // the handle, from here on
    if (a->value == 2) return fail(DCOMP_EUNSUPPORTED, "%s: the actor's value function is shared (vf_share_layers=True): the learner needs a value trunk of its own", fn);
    if (a->value != 1) return fail(DCOMP_EINVAL, "%s: the actor has no value trunk (dcomp_actor_set_value with shared = 0)", fn);

    if (int rc = check_device(fn, "the actor lives", a->device)) return rc;

    const Net &n = a->net;
    const ActorPlan &apl = a->plan;
    const int Hp = apl.Hp, KS2 = apl.KS2, NT3 = apl.NT3;
    dcomp_learner *l = new dcomp_learner();
    memset(l, 0, sizeof(*l));
    l->a = a; l->max_rows = cfg->max_rows; l->device = a->device;
    const LearnerPlan &pl = l->plan = learner_plan(apl);
    l->ld = pl.ld_of(cfg->max_rows);
    l->beta1 = cfg->beta1; l->beta2 = cfg->beta2; l->eps = cfg->eps;
    const int total = pl.total;

    // one allocation: flat f32 arrays | backward fragments | activation / delta workspaces | walk and statistics workspaces | partials
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = up(at + bytes); return o; };
    const size_t o_flat = take((size_t)4 * total * 4);
    const size_t n_w2b = (size_t)apl.mt * KS2 * 512, n_w3b = (size_t)apl.mt * 2 * NT3 * 512, n_vw3b = (size_t)apl.mt * 2 * 512;
    const size_t o_w2b = take(n_w2b * 2), o_w3b = take(n_w3b * 2), o_vw2b = take(n_w2b * 2), o_vw3b = take(n_vw3b * 2);
    const size_t zero_end = at;                                                      // (zeroed up to here and over X: padding must read as zero)
    const size_t ld = (size_t)l->ld;
    const size_t o_X = take((size_t)pl.K1pp * ld * 2);
    size_t o_H[8];
    for (int i = 0; i < 8; i++) o_H[i] = take((size_t)Hp * ld * 2);
    const size_t o_D3 = take((size_t)pl.N3p * ld * 2), o_VD3 = take((size_t)32 * ld * 2);
    const size_t o_head = take((size_t)cfg->max_rows * apl.heads * 16), o_tpart = take((ld / 32) * 32);      // (ld / 32 >= the tiles of max_rows)
    size_t o_part[6], o_bpart[6];
    for (int i = 0; i < 6; i++) { o_part[i] = take((size_t)MAX_CHUNKS * pl.in_p[i] * pl.out_p[i] * 4); o_bpart[i] = take((size_t)MAX_CHUNKS * pl.out_p[i] * 4); }
    l->norm_parts = (total + NORM_SPAN - 1) / NORM_SPAN;
    const size_t o_norm = take((size_t)l->norm_parts * 8);
    const size_t bytes = at;

    hipError_t e = hipMalloc(&l->mem, bytes);
    unsigned char *d = static_cast<unsigned char *>(l->mem);
    if (e == hipSuccess) e = hipMemset(d, 0, zero_end);
    if (e == hipSuccess) e = hipMemset(d + o_X, 0, (size_t)pl.K1pp * ld * 2);
    float *src[NARR];
    members(cfg->weights, src);
    l->w = reinterpret_cast<float *>(d + o_flat); l->g = l->w + total; l->m = l->g + total; l->v = l->m + total;
    l->norm_part = reinterpret_cast<double *>(d + o_norm);
    for (int i = 0; i < NARR && e == hipSuccess; i++) e = hipMemcpy(l->w + pl.off[i], src[i], (size_t)pl.len[i] * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (l->mem) (void)hipFree(l->mem);
        delete l;
        return fail(DCOMP_EHIP, "%s: %s (%zu bytes of device memory for max_rows %lld)", fn, hipGetErrorString(e), bytes, (long long)cfg->max_rows);
    }

    LParams &p = l->lp;
    p.net = n;
    p.w2b = reinterpret_cast<const uint4 *>(d + o_w2b); p.w3b = reinterpret_cast<const uint4 *>(d + o_w3b);
    p.vw2b = reinterpret_cast<const uint4 *>(d + o_vw2b); p.vw3b = reinterpret_cast<const uint4 *>(d + o_vw3b);
    auto bf = [&](size_t o) { return reinterpret_cast<__bf16 *>(d + o); };
    p.X = bf(o_X); p.H1 = bf(o_H[0]); p.H2 = bf(o_H[1]); p.D1 = bf(o_H[2]); p.D2 = bf(o_H[3]);
    p.VH1 = bf(o_H[4]); p.VH2 = bf(o_H[5]); p.VD1 = bf(o_H[6]); p.VD2 = bf(o_H[7]); p.D3 = bf(o_D3); p.VD3 = bf(o_VD3);
    p.headws = reinterpret_cast<float4 *>(d + o_head); p.part = reinterpret_cast<double *>(d + o_tpart);
    p.ld = l->ld;

    WParams &w = l->wp;
    const __bf16 *wa[6] = {p.X, p.H1, p.H2, p.X, p.VH1, p.VH2}, *wd[6] = {p.D1, p.D2, p.D3, p.VD1, p.VD2, p.VD3};
    for (int i = 0; i < 6; i++) {
        w.g[i].a = wa[i]; w.g[i].d = wd[i];
        w.g[i].part = reinterpret_cast<float *>(d + o_part[i]); w.g[i].bpart = reinterpret_cast<float *>(d + o_bpart[i]);
        w.g[i].mi_tiles = pl.in_p[i] / 32; w.g[i].ni_tiles = pl.out_p[i] / 32; w.g[i].first_task = pl.first_task[i]; w.g[i].nmain = pl.nmain[i];
    }
    w.ld = l->ld; w.ntask = pl.ntask;

    AParams &ap = l->ap;
    ap.total = total; ap.w = l->w; ap.g = l->g; ap.m = l->m; ap.v = l->v; ap.tile_part = p.part;
    auto u16 = [](const void *q) { return reinterpret_cast<uint16_t *>(const_cast<void *>(q)); };
    auto f32 = [](const float *q) { return const_cast<float *>(q); };
    for (int i = 0; i < NARR; i++) {
        ADesc &x = ap.a[i];
        const int layer = i / 2;                                                     // 0 ... 5: the weight-gradient products
        x.off = pl.off[i]; x.nin = pl.nin[i]; x.nout = pl.nout[i]; x.in_p = pl.in_p[layer]; x.out_p = pl.out_p[layer]; x.is_bias = i & 1;
        x.part = (i & 1) ? w.g[layer].bpart : w.g[layer].part;
    }
    const Trunk *trunk[2] = {&n.pi, &n.vf};
    const uint4 *w2b[2] = {p.w2b, p.vw2b}, *w3b[2] = {p.w3b, p.vw3b};
    for (int t = 0; t < 2; t++) {
        ADesc *x = ap.a + 6 * t;                                                     // w1 b1 w2 b2 w3 b3 of the trunk
        x[0].fwd = u16(trunk[t]->w1); x[0].fwd_ks = apl.K1p / 16; x[0].fwd_perm = 0;
        x[2].fwd = u16(trunk[t]->w2); x[2].fwd_ks = KS2; x[2].fwd_perm = 1; x[2].bwd = u16(w2b[t]); x[2].bwd_ks = KS2; x[2].bwd_perm = 1;
        x[4].fwd = u16(trunk[t]->w3); x[4].fwd_ks = KS2; x[4].fwd_perm = 1; x[4].bwd = u16(w3b[t]); x[4].bwd_ks = t ? 2 : 2 * NT3; x[4].bwd_perm = 0;
        x[1].bias = f32(trunk[t]->b1); x[3].bias = f32(trunk[t]->b2); x[5].bias = f32(trunk[t]->b3);
    }

    launch_adam(l, false, 0.f, nullptr);                                             // the backward fragments (and the forward ones, again) from the masters
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipFree(l->mem);
        delete l;
        return fail(DCOMP_EHIP, "%s: %s", fn, hipGetErrorString(e));
    }
    *out = l;
    return DCOMP_OK;
}

extern "C" int dcomp_learner_destroy(dcomp_learner *l)
{
    if (!l) return DCOMP_OK;
    const hipError_t e = hipFree(l->mem);
    delete l;
    return e == hipSuccess ? DCOMP_OK : fail(DCOMP_EHIP, "dcomp_learner_destroy: hipFree failed: %s", hipGetErrorString(e));
}

// One (mini)batch as both surfaces give it: dcomp_ppo_batch (dcomp_learner.h: position i is row i of the pointers) and
// dcomp_sgd_batch (dcomp_learner_indexed.h: position i is source row index[i] of a whole sample batch, rows or compact record).
struct BatchView {
    bool indexed;
    int32_t obs_format, num_active;
    int64_t rows, source_rows;
    const int32_t *index;
    const void *obs;
    const uint8_t *actions;
    const float *old_logp, *old_logits, *advantages, *value_targets, *old_vf;
    float *logp, *entropy, *kl, *vf, *ratio;
    const float *dlogits, *dvalue;
};

// every host check of a grads (evaluate = false) or evaluate call on one learner; the grouped call makes them per policy
static int learner_check(const char *fn, bool evaluate, const dcomp_learner *l, const BatchView *b, const dcomp_ppo_hyper *hy, const float *stats)
{
    if (!evaluate) {
        if (!hy) return fail(DCOMP_EINVAL, "%s: hyper must not be NULL", fn);
        if (int rc = check_struct(fn, "dcomp_ppo_hyper", hy->struct_size, sizeof(dcomp_ppo_hyper))) return rc;
        if (!stats) return fail(DCOMP_EINVAL, "%s: stats_dev must not be NULL", fn);
        if (!(hy->clip_param >= 0.f) || !(hy->vf_clip_param >= 0.f)) return fail(DCOMP_EINVAL, "%s: clip_param %g / vf_clip_param %g must be >= 0", fn, hy->clip_param, hy->vf_clip_param);
    }
    const bool compact = b->indexed && b->obs_format == DCOMP_ACTOR_COMPACT;
    if (b->obs_format == DCOMP_ACTOR_COMPACT && !b->indexed)
        return fail(DCOMP_EUNSUPPORTED, "%s: the compact record is not supported as learner input: pass observation rows", fn);
    if (b->obs_format != DCOMP_ACTOR_ROWS && !compact) return fail(DCOMP_EINVAL, "%s: unknown obs_format %d", fn, b->obs_format);
    if (!b->obs) return fail(DCOMP_EINVAL, "%s: batch.obs must not be NULL", fn);
    const bool upstream = b->dlogits || b->dvalue;
    if (evaluate) {
        if (!b->actions) return fail(DCOMP_EINVAL, "%s: batch.actions must not be NULL", fn);
        if (!b->logp && !b->entropy && !b->vf) return fail(DCOMP_EINVAL, "%s: none of batch.logp / entropy / vf is given: nothing to write", fn);
        if (upstream) return fail(DCOMP_EINVAL, "%s: upstream gradients (batch.dlogits / dvalue) belong to the grads call", fn);
    } else if (upstream) {
        if (!b->dlogits || !b->dvalue) return fail(DCOMP_EINVAL, "%s: batch.dlogits and batch.dvalue come together: one of them is NULL", fn);
    } else if (!b->actions || !b->old_logp || !b->old_logits || !b->advantages || !b->value_targets || !b->old_vf) {
        return fail(DCOMP_EINVAL, "%s: a pointer of batch.actions / old_logp / old_logits / advantages / value_targets / old_vf is NULL", fn);
    }
    if (b->rows < 1) return fail(DCOMP_EINVAL, "%s: rows %lld < 1", fn, (long long)b->rows);
    if (b->indexed) {
        if (b->source_rows < 1 || b->source_rows > 0x7FFFFFFFll)
            return fail(DCOMP_EINVAL, "%s: source_rows %lld outside [1, 2^31 - 1]", fn, (long long)b->source_rows);
        if (!b->index && b->rows > b->source_rows)
            return fail(DCOMP_EINVAL, "%s: without an index position i reads source row i: rows %lld > source_rows %lld", fn, (long long)b->rows, (long long)b->source_rows);
    }
    // the handle, from here on
    if (b->rows > l->max_rows) return fail(DCOMP_EINVAL, "%s: rows %lld > max_rows %lld of the handle", fn, (long long)b->rows, (long long)l->max_rows);
    const dcomp_actor *a = l->a;
    const int U = a->net.U;
    if (compact && !a->net.multi) return fail(DCOMP_EUNSUPPORTED, "%s: the compact record exists for multi-agent observations only", fn);
    if (compact && b->source_rows % U)
        return fail(DCOMP_EINVAL, "%s: the compact record holds whole envs: source_rows %lld is not a multiple of num_ue %d", fn, (long long)b->source_rows, U);
    if (b->num_active < 0 || b->num_active > U) return fail(DCOMP_EINVAL, "%s: num_active %d outside [0, %d]", fn, b->num_active, U);
    if (b->indexed && a->net.multi && b->num_active != U)
        return fail(DCOMP_EINVAL, "%s: num_active %d != num_ue %d: with multi-agent rows select the listed rows through the index (every position counts in 1 / N)", fn, b->num_active, U);
    return DCOMP_OK;
}

// the grads and evaluate calls of both surfaces: every check on the host first.  acc / sums (dcomp_learner_accum.h, both or
// neither; grads only): the chunk partials go into the caller's running sum instead of the handle's gradients
static int learner_launch(const char *fn, bool evaluate, dcomp_learner *l, const BatchView *b, const dcomp_ppo_hyper *hy, float *stats, void *stream,
                          float *acc = nullptr, double *sums = nullptr)
{
    using namespace dlearn;
    if (int rc = learner_check(fn, evaluate, l, b, hy, stats)) return rc;
    const dcomp_actor *a = l->a;
    const int U = a->net.U;
    const bool compact = b->indexed && b->obs_format == DCOMP_ACTOR_COMPACT, upstream = b->dlogits || b->dvalue;

    hipStream_t s = static_cast<hipStream_t>(stream);
    LParams p = l->lp;
    p.obs = static_cast<const float *>(b->obs); p.actions = b->actions; p.old_logp = b->old_logp; p.old_logits = b->old_logits; p.adv = b->advantages;
    p.vtarg = b->value_targets; p.old_vf = b->old_vf;
    p.o_logp = b->logp; p.o_ent = b->entropy; p.o_kl = b->kl; p.o_vf = b->vf; p.o_ratio = b->ratio;
    p.up_dlogits = b->dlogits; p.up_dvalue = b->dvalue;
    const RowSplit rs = row_split(b->rows);
    p.rows = b->rows; p.tiles = rs.tiles; p.num_active = b->num_active;
    p.fwd_only = evaluate; p.upstream = upstream;
    if (hy) { p.clip = hy->clip_param; p.vf_clip = hy->vf_clip_param; p.vf_coeff = hy->vf_loss_coeff; p.ent_coeff = hy->entropy_coeff; p.kl_coeff = hy->kl_coeff; }
    const int grid = launch_blocks(p.tiles, a->max_blocks);
    const size_t lds = (size_t)a->plan.lds_per_wave * WAVES;
    if (b->indexed) {
        IParams ip;
        static_cast<LParams &>(ip) = p;
        ip.index = b->index; ip.source_rows = b->source_rows; ip.compact = compact;
        hipLaunchKernelGGL(pick_indexed(a->plan.mt, a->relu != 0), dim3(grid), dim3(BLOCK), lds, s, ip);
    } else {
        hipLaunchKernelGGL(pick(a->plan.mt, a->relu != 0), dim3(grid), dim3(BLOCK), lds, s, p);
    }
    HIP_TRY(hipGetLastError());
    if (evaluate) return DCOMP_OK;

    WParams w = l->wp;
    w.rows_pad = rs.rows_pad; w.chunk_rows = rs.chunk_rows;
    hipLaunchKernelGGL(wgrad_kernel, dim3((w.ntask + WAVES - 1) / WAVES, rs.nchunks), dim3(BLOCK), 0, s, w);
    HIP_TRY(hipGetLastError());

    AParams ap = l->ap;
    ap.nchunks = rs.nchunks; ap.tiles = p.tiles; ap.stats = stats; ap.want_stats = 1;
    // the count behind 1 / N, on the host: indexed, every position (the index's contents cannot change it)
    const int64_t counted = b->indexed || !a->net.multi ? b->rows : (b->rows / U) * b->num_active + (b->rows % U < b->num_active ? b->rows % U : b->num_active);
    ap.count = upstream ? 0. : (double)counted;
    ap.scale = upstream ? 1.f : (counted > 0 ? (float)(1.0 / (double)counted) : 0.f);
    ap.vf_coeff = p.vf_coeff; ap.ent_coeff = p.ent_coeff; ap.kl_coeff = p.kl_coeff;
    if (acc) hipLaunchKernelGGL(accumulate_kernel, dim3((l->plan.total + 255) / 256), dim3(256), 0, s, ap, acc, sums);
    else hipLaunchKernelGGL(reduce_kernel, dim3((l->plan.total + 255) / 256), dim3(256), 0, s, ap);
    HIP_TRY(hipGetLastError());
    return DCOMP_OK;
}

// the NULL and struct-size checks of a surface's batch, then its view
static int ppo_launch(const char *fn, bool evaluate, dcomp_learner *l, const dcomp_ppo_batch *b, const dcomp_ppo_hyper *hy, float *stats, void *stream,
                      float *acc = nullptr, double *sums = nullptr)
{
    if (!l || !b) return fail(DCOMP_EINVAL, "%s: handle and batch must not be NULL", fn);
    if (int rc = check_struct(fn, "dcomp_ppo_batch", b->struct_size, sizeof(dcomp_ppo_batch))) return rc;
    const BatchView v = {false, b->obs_format, b->num_active, b->rows, b->rows, nullptr, b->obs, b->actions, b->old_logp, b->old_logits, b->advantages,
                         b->value_targets, b->old_vf, b->logp, b->entropy, b->kl, b->vf, b->ratio, b->dlogits, b->dvalue};
    return learner_launch(fn, evaluate, l, &v, hy, stats, stream, acc, sums);
}

static int sgd_launch(const char *fn, bool evaluate, dcomp_learner *l, const dcomp_sgd_batch *b, const dcomp_ppo_hyper *hy, float *stats, void *stream,
                      float *acc = nullptr, double *sums = nullptr)
{
    if (!l || !b) return fail(DCOMP_EINVAL, "%s: handle and batch must not be NULL", fn);
    if (int rc = check_struct(fn, "dcomp_sgd_batch", b->struct_size, sizeof(dcomp_sgd_batch))) return rc;
    const BatchView v = {true, b->obs_format, b->num_active, b->rows, b->source_rows, b->index, b->obs, b->actions, b->old_logp, b->old_logits, b->advantages,
                         b->value_targets, b->old_vf, b->logp, b->entropy, b->kl, b->vf, b->ratio, b->dlogits, b->dvalue};
    return learner_launch(fn, evaluate, l, &v, hy, stats, stream, acc, sums);
}

extern "C" int dcomp_learner_grads(dcomp_learner *l, const dcomp_ppo_batch *b, const dcomp_ppo_hyper *hy, float *stats_dev, void *stream)
{
    return ppo_launch("dcomp_learner_grads", false, l, b, hy, stats_dev, stream);
}

extern "C" int dcomp_learner_evaluate(dcomp_learner *l, const dcomp_ppo_batch *b, void *stream)
{
    return ppo_launch("dcomp_learner_evaluate", true, l, b, nullptr, nullptr, stream);
}

extern "C" int dcomp_sgd_grads(dcomp_learner *l, const dcomp_sgd_batch *b, const dcomp_ppo_hyper *hy, float *stats_dev, void *stream)
{
    return sgd_launch("dcomp_sgd_grads", false, l, b, hy, stats_dev, stream);
}

extern "C" int dcomp_sgd_evaluate(dcomp_learner *l, const dcomp_sgd_batch *b, void *stream)
{
    return sgd_launch("dcomp_sgd_evaluate", true, l, b, nullptr, nullptr, stream);
}

// ---------------------------------------------------------------- include/dcomp_learner_accum.h
extern "C" int dcomp_learner_flat_size(const dcomp_learner *l, int64_t *floats)
{
    if (!l || !floats) return fail(DCOMP_EINVAL, "dcomp_learner_flat_size: handle and floats must not be NULL");
    *floats = l->plan.total;
    return DCOMP_OK;
}

// what the accumulate calls check beyond learner_check (which sees sums_dev where the grads calls have stats_dev: non-NULL by then)
template <class B> static int accumulate_check(const char *fn, const dcomp_learner *l, const B *b, const float *acc, const double *sums)
{
    if (!l || !b) return fail(DCOMP_EINVAL, "%s: handle and batch must not be NULL", fn);
    if (!acc || !sums) return fail(DCOMP_EINVAL, "%s: acc_dev and sums_dev must not be NULL", fn);
    if (b->struct_size == (int32_t)sizeof(B) && (b->dlogits || b->dvalue))
        return fail(DCOMP_EINVAL, "%s: upstream gradients (batch.dlogits / dvalue) are plain sums already: they belong to the grads call", fn);
    return DCOMP_OK;
}

extern "C" int dcomp_learner_accumulate(dcomp_learner *l, const dcomp_ppo_batch *b, const dcomp_ppo_hyper *hy, float *acc_dev, double *sums_dev, void *stream)
{
    const char *fn = "dcomp_learner_accumulate";
    if (int rc = accumulate_check(fn, l, b, acc_dev, sums_dev)) return rc;
    return ppo_launch(fn, false, l, b, hy, reinterpret_cast<float *>(sums_dev), stream, acc_dev, sums_dev);
}

extern "C" int dcomp_sgd_accumulate(dcomp_learner *l, const dcomp_sgd_batch *b, const dcomp_ppo_hyper *hy, float *acc_dev, double *sums_dev, void *stream)
{
    const char *fn = "dcomp_sgd_accumulate";
    if (int rc = accumulate_check(fn, l, b, acc_dev, sums_dev)) return rc;
    return sgd_launch(fn, false, l, b, hy, reinterpret_cast<float *>(sums_dev), stream, acc_dev, sums_dev);
}

extern "C" int dcomp_learner_accum_finish(dcomp_learner *l, const float *acc_dev, const double *sums_dev, const dcomp_ppo_hyper *hy, float grad_clip,
                                          float *stats_dev, float *grad_norm_dev, void *stream)
{
    using namespace dlearn;
    const char *fn = "dcomp_learner_accum_finish";
    if (!l) return fail(DCOMP_EINVAL, "%s: handle must not be NULL", fn);
    if (!acc_dev || !sums_dev) return fail(DCOMP_EINVAL, "%s: acc_dev and sums_dev must not be NULL", fn);
    if (!hy) return fail(DCOMP_EINVAL, "%s: hyper must not be NULL", fn);
    if (int rc = check_struct(fn, "dcomp_ppo_hyper", hy->struct_size, sizeof(dcomp_ppo_hyper))) return rc;
    if (!(grad_clip >= 0.f)) return fail(DCOMP_EINVAL, "%s: grad_clip %g must be >= 0 (0: no clipping)", fn, grad_clip);
    // the handle, from here on
    hipStream_t s = static_cast<hipStream_t>(stream);
    FParams p;
    p.acc = acc_dev; p.sums = sums_dev; p.g = l->g; p.stats = stats_dev; p.grad_norm = grad_norm_dev; p.norm_part = l->norm_part;
    p.total = l->plan.total; p.nparts = l->norm_parts; p.want_norm = grad_clip > 0.f || grad_norm_dev;
    p.clip = grad_clip; p.vf_coeff = hy->vf_loss_coeff; p.ent_coeff = hy->entropy_coeff; p.kl_coeff = hy->kl_coeff;
    if (p.want_norm) {
        hipLaunchKernelGGL(norm_kernel, dim3(p.nparts), dim3(256), 0, s, p);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(finish_kernel, dim3((p.total + 255) / 256), dim3(256), 0, s, p);
    HIP_TRY(hipGetLastError());
    return DCOMP_OK;
}

extern "C" int dcomp_learner_apply(dcomp_learner *l, float lr, void *stream)
{
    if (!l) return fail(DCOMP_EINVAL, "dcomp_learner_apply: handle must not be NULL");
    if (!(lr >= 0.f) || !std::isfinite(lr)) return fail(DCOMP_EINVAL, "dcomp_learner_apply: lr %g is not a finite number >= 0", lr);
    launch_adam(l, true, lr, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    l->step++;
    return DCOMP_OK;
}

extern "C" int dcomp_learner_read(dcomp_learner *l, int32_t which, const dcomp_learner_arrays *dst, int64_t *step, void *stream)
{
    const char *fn = "dcomp_learner_read";
    if (!l) return fail(DCOMP_EINVAL, "%s: handle must not be NULL", fn);
    if (which < DCOMP_LEARNER_WEIGHTS || which > DCOMP_LEARNER_ADAM_V) return fail(DCOMP_EINVAL, "%s: which %d is not one of DCOMP_LEARNER_*", fn, which);
    if (int rc = check_arrays(fn, "dst", dst, false)) return rc;
    const float *src = which == DCOMP_LEARNER_WEIGHTS ? l->w : which == DCOMP_LEARNER_GRADS ? l->g : which == DCOMP_LEARNER_ADAM_M ? l->m : l->v;
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    float *m[dlearn::NARR];
    members(dst, m);
    for (int i = 0; i < dlearn::NARR; i++)
        if (m[i]) HIP_TRY(hipMemcpy(m[i], src + l->plan.off[i], (size_t)l->plan.len[i] * 4, hipMemcpyDeviceToHost));
    if (step) *step = l->step;
    return DCOMP_OK;
}

extern "C" int dcomp_learner_load_state(dcomp_learner *l, const dcomp_learner_arrays *weights, const dcomp_learner_arrays *adam_m,
                                        const dcomp_learner_arrays *adam_v, int64_t step, void *stream)
{
    const char *fn = "dcomp_learner_load_state";
    if (!l) return fail(DCOMP_EINVAL, "%s: handle must not be NULL", fn);
    if (int rc = check_arrays(fn, "weights", weights, true)) return rc;
    if (int rc = check_arrays(fn, "adam_m", adam_m, true)) return rc;
    if (int rc = check_arrays(fn, "adam_v", adam_v, true)) return rc;
    if (step < 0) return fail(DCOMP_EINVAL, "%s: step %lld < 0", fn, (long long)step);
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipStreamSynchronize(s));
    const dcomp_learner_arrays *from[3] = {weights, adam_m, adam_v};
    float *to[3] = {l->w, l->m, l->v};
    for (int k = 0; k < 3; k++) {
        float *m[dlearn::NARR];
        members(from[k], m);
        for (int i = 0; i < dlearn::NARR; i++) HIP_TRY(hipMemcpy(to[k] + l->plan.off[i], m[i], (size_t)l->plan.len[i] * 4, hipMemcpyHostToDevice));
    }
    l->step = step;
    launch_adam(l, false, 0.f, s);
    HIP_TRY(hipGetLastError());
    return DCOMP_OK;
}

// ---------------------------------------------------------------- a group of learners (include/dcomp_learner_group.h)
struct dcomp_learner_group {
    std::vector<dcomp_learner *> members;
    int32_t device;
    dlearn::GEntry *table;                // [members]: device
};

extern "C" int dcomp_learner_group_create(const dcomp_learner_group_cfg *cfg, dcomp_learner_group **out)
{
    using namespace dlearn;
    const char *fn = "dcomp_learner_group_create";
    if (out) *out = nullptr;
    if (!cfg || !out) return fail(DCOMP_EINVAL, "%s: cfg and out must not be NULL", fn);
    if (int rc = check_struct(fn, "dcomp_learner_group_cfg", cfg->struct_size, sizeof(dcomp_learner_group_cfg))) return rc;
    if (!cfg->learners) return fail(DCOMP_EINVAL, "%s: learners must not be NULL", fn);
    const int P = cfg->num_learners;
    if (P < 1 || P > DCOMP_MAX_UE) return fail(DCOMP_EINVAL, "%s: num_learners %d outside [1, %d]", fn, P, DCOMP_MAX_UE);
    for (int i = 0; i < P; i++) {
        if (!cfg->learners[i]) return fail(DCOMP_EINVAL, "%s: learner %d is NULL", fn, i);
        for (int j = 0; j < i; j++)
            if (cfg->learners[j] == cfg->learners[i]) return fail(DCOMP_EINVAL, "%s: learner %d is learner %d again: a member is listed once", fn, i, j);
    }
    // the members, from here on
    for (int i = 0; i < P; i++)
        for (int j = 0; j < i; j++)
            if (cfg->learners[j]->a == cfg->learners[i]->a) return fail(DCOMP_EINVAL, "%s: learners %d and %d train the same actor", fn, j, i);
    const dcomp_learner *f = cfg->learners[0];
    for (int i = 1; i < P; i++) {
        const dcomp_learner *m = cfg->learners[i];
        const struct { const char *what; int a, b; } same[] = {
            {"obs_kind", f->a->net.multi, m->a->net.multi}, {"num_ue", f->a->net.U, m->a->net.U}, {"num_bs", f->a->net.B, m->a->net.B},
            {"hidden", f->a->plan.hidden, m->a->plan.hidden}, {"activation", f->a->relu, m->a->relu}, {"device", f->device, m->device}};
        for (const auto &c : same)
            if (c.a != c.b) return fail(DCOMP_EINVAL, "%s: learner %d differs from learner 0 in %s (%d, %d)", fn, i, c.what, c.b, c.a);
    }
    if (!f->a->net.multi) return fail(DCOMP_EUNSUPPORTED, "%s: DCOMP_CENTRAL learners: a central policy is one network by construction", fn);
    if (int rc = check_device(fn, "the learners live", f->device)) return rc;

    std::vector<GEntry> host((size_t)P);
    for (int i = 0; i < P; i++) {
        const dcomp_learner *m = cfg->learners[i];
        GEntry &e = host[(size_t)i];
        memset(&e, 0, sizeof(e));
        e.lp = m->lp;
        for (int k = 0; k < 6; k++) e.wg[k] = m->wp.g[k];
        for (int k = 0; k < NARR; k++) e.a[k] = m->ap.a[k];
        e.w = m->w; e.g = m->g; e.m = m->m; e.v = m->v;
        e.total = m->plan.total; e.ntask = m->plan.ntask;
        e.beta1 = m->beta1; e.beta2 = m->beta2; e.eps = m->eps;
        e.omb1 = (float)(1.0 - (double)m->beta1); e.omb2 = (float)(1.0 - (double)m->beta2);      // (as launch_adam)
        e.norm_part = m->norm_part; e.norm_parts = m->norm_parts;
    }
    dcomp_learner_group *g = new dcomp_learner_group();
    g->members.assign(cfg->learners, cfg->learners + P);
    g->device = f->device; g->table = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&g->table), host.size() * sizeof(GEntry));
    if (e == hipSuccess) {
        e = hipMemcpy(g->table, host.data(), host.size() * sizeof(GEntry), hipMemcpyHostToDevice);
        if (e != hipSuccess) (void)hipFree(g->table);
    }
    if (e != hipSuccess) {
        delete g;
        return fail(DCOMP_EHIP, "%s: %s", fn, hipGetErrorString(e));
    }
    *out = g;
    return DCOMP_OK;
}

extern "C" int dcomp_learner_group_destroy(dcomp_learner_group *g)
{
    if (!g) return DCOMP_OK;
    const hipError_t e = hipFree(g->table);
    delete g;
    return e == hipSuccess ? DCOMP_OK : fail(DCOMP_EHIP, "dcomp_learner_group_destroy: hipFree failed: %s", hipGetErrorString(e));
}

// the grads and accumulate calls of a group: every check on the host first.  acc / sums (dcomp_learner_group_accum.h, both or neither):
// the chunk partials go into the caller's [P][flat] running sums instead of the handles' gradients; the callers have checked their
// own pointers (stats_dev stands for sums_dev there: non-NULL by then)
static int group_launch(const char *fn, dcomp_learner_group *g, const dcomp_group_batch *b, const dcomp_ppo_hyper *hyper, float *stats_dev, void *stream,
                        float *acc = nullptr, double *sums = nullptr)
{
    using namespace dlearn;
    if (int rc = check_struct(fn, "dcomp_group_batch", b->struct_size, sizeof(dcomp_group_batch))) return rc;
    if (!b->rows || !b->index) return fail(DCOMP_EINVAL, "%s: batch.rows and batch.index must not be NULL", fn);
    const int P = (int)g->members.size();
    int active = 0;
    for (int i = 0; i < P; i++) {
        const dcomp_learner *m = g->members[(size_t)i];
        const int64_t r = b->rows[i];
        if (r < 0 || r > m->max_rows) return fail(DCOMP_EINVAL, "%s: rows[%d] %lld outside [0, max_rows %lld of the learner]", fn, i, (long long)r, (long long)m->max_rows);
        if (r > b->index_stride) return fail(DCOMP_EINVAL, "%s: rows[%d] %lld > index_stride %lld", fn, i, (long long)r, (long long)b->index_stride);
        if (r == 0) continue;
        active++;
        // one policy's call as dcomp_sgd_grads would see it: its checks are learner_launch's
        const BatchView v = {true, b->obs_format, m->a->net.U, r, b->source_rows, b->index + (int64_t)i * b->index_stride, b->obs, b->actions, b->old_logp,
                             b->old_logits, b->advantages, b->value_targets, b->old_vf, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (int rc = learner_check(fn, false, m, &v, hyper + i, stats_dev)) return rc;
    }
    if (!active) return fail(DCOMP_EINVAL, "%s: every rows[p] is 0: at least one policy must take part", fn);
    if (int rc = check_device(fn, "the group lives", g->device)) return rc;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const dcomp_learner *f = g->members[0];
    const dcomp_actor *a = f->a;
    const size_t lds = (size_t)a->plan.lds_per_wave * WAVES;
    const group_fn kernel = pick_group(a->plan.mt, a->relu != 0);
    for (int first = 0; first < P; first += GROUP_SLICE) {
        const int n = P - first < GROUP_SLICE ? P - first : GROUP_SLICE;
        GLParams lp;
        GWParams wp;
        GRParams rp;
        GCParams cp;
        memset(&lp, 0, sizeof(lp)); memset(&wp, 0, sizeof(wp)); memset(&rp, 0, sizeof(rp)); memset(&cp, 0, sizeof(cp));
        int64_t max_rows = 0;
        int nactive = 0;
        for (int i = 0; i < n; i++) {
            const int64_t r = b->rows[first + i];
            const dcomp_ppo_hyper &hy = hyper[first + i];
            lp.rows[i] = wp.rows[i] = rp.rows[i] = cp.rows[i] = (int32_t)r;          // (<= max_rows <= 2^28)
            lp.clip[i] = hy.clip_param; lp.vf_clip[i] = hy.vf_clip_param;
            lp.vf_coeff[i] = rp.vf_coeff[i] = hy.vf_loss_coeff; lp.ent_coeff[i] = rp.ent_coeff[i] = hy.entropy_coeff; lp.kl_coeff[i] = rp.kl_coeff[i] = hy.kl_coeff;
            rp.scale[i] = r > 0 ? (float)(1.0 / (double)r) : 0.f;                   // learner_launch's 1 / N: indexed, every position counts
            if (r > 0) nactive++;
            if (r > max_rows) max_rows = r;
        }
        if (!nactive) continue;
        // the tile axis is sized by the slice's largest policy (tiles grow with rows); the chunk axis by the largest CHUNK COUNT, which
        // is not the largest policy's: past CHUNK_UNIT x MAX_CHUNKS rows the chunks get longer and fewer (group_chunks)
        const int64_t max_tiles = tiles_of(max_rows);
        const int max_chunks = group_chunks(b->rows + first, n);
        lp.obs = static_cast<const float *>(b->obs); lp.actions = b->actions; lp.old_logp = b->old_logp; lp.old_logits = b->old_logits;
        lp.adv = b->advantages; lp.vtarg = b->value_targets; lp.old_vf = b->old_vf;
        lp.table = wp.table = rp.table = cp.table = g->table + first;
        lp.index = b->index + (int64_t)first * b->index_stride; lp.index_stride = b->index_stride; lp.source_rows = b->source_rows;
        lp.compact = b->obs_format == DCOMP_ACTOR_COMPACT; lp.num_active = a->net.U;
        rp.stats = stats_dev + (size_t)first * DCOMP_PPO_NUM_STATS;
        hipLaunchKernelGGL(kernel, dim3(group_blocks(max_tiles, a->max_blocks, nactive), n), dim3(BLOCK), lds, s, lp);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(wgrad_group_kernel, dim3((f->plan.ntask + WAVES - 1) / WAVES, max_chunks, n), dim3(BLOCK), 0, s, wp);
        HIP_TRY(hipGetLastError());
        if (acc) {
            cp.acc = acc + (size_t)first * (size_t)f->plan.total; cp.sums = sums + (size_t)first * DCOMP_ACCUM_SUMS;
            hipLaunchKernelGGL(accumulate_group_kernel, dim3((f->plan.total + 255) / 256, n), dim3(256), 0, s, cp);
        } else {
            hipLaunchKernelGGL(reduce_group_kernel, dim3((f->plan.total + 255) / 256, n), dim3(256), 0, s, rp);
        }
        HIP_TRY(hipGetLastError());
    }
    return DCOMP_OK;
}

extern "C" int dcomp_learner_group_grads(dcomp_learner_group *g, const dcomp_group_batch *b, const dcomp_ppo_hyper *hyper, float *stats_dev, void *stream)
{
    const char *fn = "dcomp_learner_group_grads";
    if (!g || !b || !hyper || !stats_dev) return fail(DCOMP_EINVAL, "%s: group, batch, hyper and stats_dev must not be NULL", fn);
    return group_launch(fn, g, b, hyper, stats_dev, stream);
}

// ---------------------------------------------------------------- include/dcomp_learner_group_accum.h
extern "C" int dcomp_learner_group_accumulate(dcomp_learner_group *g, const dcomp_group_batch *b, const dcomp_ppo_hyper *hyper, float *acc_dev,
                                              double *sums_dev, void *stream)
{
    const char *fn = "dcomp_learner_group_accumulate";
    if (!g || !b || !hyper) return fail(DCOMP_EINVAL, "%s: group, batch and hyper must not be NULL", fn);
    if (!acc_dev || !sums_dev) return fail(DCOMP_EINVAL, "%s: acc_dev and sums_dev must not be NULL", fn);
    return group_launch(fn, g, b, hyper, reinterpret_cast<float *>(sums_dev), stream, acc_dev, sums_dev);
}

extern "C" int dcomp_learner_group_accum_finish(dcomp_learner_group *g, const float *acc_dev, const double *sums_dev, const dcomp_ppo_hyper *hyper,
                                                const float *grad_clip, const int32_t *active, float *stats_dev, float *grad_norm_dev, void *stream)
{
    using namespace dlearn;
    const char *fn = "dcomp_learner_group_accum_finish";
    if (!g) return fail(DCOMP_EINVAL, "%s: group must not be NULL", fn);
    if (!acc_dev || !sums_dev) return fail(DCOMP_EINVAL, "%s: acc_dev and sums_dev must not be NULL", fn);
    if (!hyper) return fail(DCOMP_EINVAL, "%s: hyper must not be NULL", fn);
    const int P = (int)g->members.size();
    int nactive = 0;
    for (int i = 0; i < P; i++) {
        if (active && !active[i]) continue;
        nactive++;
        if (int rc = check_struct(fn, "dcomp_ppo_hyper", hyper[i].struct_size, sizeof(dcomp_ppo_hyper))) return rc;
        if (grad_clip && !(grad_clip[i] >= 0.f)) return fail(DCOMP_EINVAL, "%s: grad_clip[%d] %g must be >= 0 (0: no clipping)", fn, i, grad_clip[i]);
    }
    if (!nactive) return fail(DCOMP_EINVAL, "%s: no member is active", fn);
    if (int rc = check_device(fn, "the group lives", g->device)) return rc;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const dcomp_learner *f = g->members[0];
    const int total = f->plan.total;
    for (int first = 0; first < P; first += GROUP_SLICE) {
        const int n = P - first < GROUP_SLICE ? P - first : GROUP_SLICE;
        GFParams fp;
        memset(&fp, 0, sizeof(fp));
        bool any = false, any_norm = false;
        for (int i = 0; i < n; i++) {
            if (active && !active[first + i]) continue;
            const dcomp_ppo_hyper &hy = hyper[first + i];
            const float clip = grad_clip ? grad_clip[first + i] : 0.f;
            fp.active[i] = 1; any = true;
            fp.clip[i] = clip; fp.want_norm[i] = clip > 0.f || grad_norm_dev;        // (dcomp_learner_accum_finish's rule)
            fp.vf_coeff[i] = hy.vf_loss_coeff; fp.ent_coeff[i] = hy.entropy_coeff; fp.kl_coeff[i] = hy.kl_coeff;
            any_norm = any_norm || fp.want_norm[i];
        }
        if (!any) continue;
        fp.table = g->table + first;
        fp.acc = acc_dev + (size_t)first * (size_t)total; fp.sums = sums_dev + (size_t)first * DCOMP_ACCUM_SUMS;
        fp.stats = stats_dev ? stats_dev + (size_t)first * DCOMP_PPO_NUM_STATS : nullptr;
        fp.grad_norm = grad_norm_dev ? grad_norm_dev + first : nullptr;
        if (any_norm) {
            hipLaunchKernelGGL(norm_group_kernel, dim3(f->norm_parts, n), dim3(256), 0, s, fp);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(finish_group_kernel, dim3((total + 255) / 256, n), dim3(256), 0, s, fp);
        HIP_TRY(hipGetLastError());
    }
    return DCOMP_OK;
}

extern "C" int dcomp_learner_group_apply(dcomp_learner_group *g, const float *lr, const int32_t *active, void *stream)
{
    using namespace dlearn;
    const char *fn = "dcomp_learner_group_apply";
    if (!g || !lr) return fail(DCOMP_EINVAL, "%s: group and lr must not be NULL", fn);
    const int P = (int)g->members.size();
    int nactive = 0;
    for (int i = 0; i < P; i++) {
        if (active && !active[i]) continue;
        nactive++;
        if (!(lr[i] >= 0.f) || !std::isfinite(lr[i])) return fail(DCOMP_EINVAL, "%s: lr[%d] %g is not a finite number >= 0", fn, i, lr[i]);
    }
    if (!nactive) return fail(DCOMP_EINVAL, "%s: no member is active", fn);
    if (int rc = check_device(fn, "the group lives", g->device)) return rc;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const int total = g->members[0]->plan.total;
    for (int first = 0; first < P; first += GROUP_SLICE) {
        const int n = P - first < GROUP_SLICE ? P - first : GROUP_SLICE;
        GAParams ap;
        memset(&ap, 0, sizeof(ap));
        ap.table = g->table + first;
        bool any = false;
        for (int i = 0; i < n; i++) {
            const dcomp_learner *m = g->members[(size_t)(first + i)];
            if (active && !active[first + i]) continue;
            const double t = (double)(m->step + 1);                                  // launch_adam's scalars, per member
            ap.active[i] = 1; any = true;
            ap.step_size[i] = (float)((double)lr[first + i] / (1.0 - std::pow((double)m->beta1, t)));
            ap.bc2_sqrt[i] = (float)std::sqrt(1.0 - std::pow((double)m->beta2, t));
        }
        if (!any) continue;
        hipLaunchKernelGGL(adam_group_kernel, dim3((total + 255) / 256, n), dim3(256), 0, s, ap);
        HIP_TRY(hipGetLastError());
        for (int i = 0; i < n; i++)
            if (ap.active[i]) g->members[(size_t)(first + i)]->step++;
    }
    return DCOMP_OK;
}
