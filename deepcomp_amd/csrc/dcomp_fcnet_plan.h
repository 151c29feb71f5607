// dcomp_fcnet_plan.h -- which instantiation, how many tiles, chunks and blocks for a shape: the fcnet kernels' host dispatch, stated
// ONCE.  dcomp_actor_create / dcomp_actor_set_value / actor_launch (dcomp_actor.hip), dcomp_learner_create / learner_launch /
// dcomp_learner_group_grads (dcomp_learner.hip) and the tests' table of cases (tests/fcnet_cases.py, through dcomp_fcnet_describe) all read it; the kernels
// read the constants and wgrad_mb / wgrad_nb.  tests/fcnet_plan_check.cpp walks every accepted shape and checks what the kernels
// rely on without saying so (K1p a multiple of 16, XS an odd number of 16-byte slots, four waves' LDS under 64 KB, ...).
//
// Plain C++17 without a HIP header: pure functions of their arguments -- no HIP call, no error text, no allocation.
// Internal: not installed, not part of the ABI.
#ifndef DCOMP_FCNET_PLAN_H
#define DCOMP_FCNET_PLAN_H

#include <cstdint>

#include "../../include/dcomp_types.h"

#ifdef __HIPCC__
#define DCOMP_PLAN_HD __host__ __device__
#else
#define DCOMP_PLAN_HD
#endif

// The constants of the plan.  The kernels' translation units spell the same names in their own namespaces where they always were
// (dcomp_actor_impl.h: dactor::WAVES ... LT; dcomp_learner.hip: dlearn::CHUNK_UNIT, MAX_CHUNKS) and static_assert them equal to these:
// a host without HIP (tests/fcnet_plan_check.cpp) cannot include those files, and a difference does not compile.
namespace dplan {

constexpr int WAVES = 4, BLOCK = WAVES * 64, TILE = 32;
constexpr int KC = 144;               // inputs staged at a time (a multiple of 16; KC + 8 elements = an odd number of 16-byte slots per row)
constexpr int LT = 33;                // row stride of the logit tile (floats): lanes walk their rows conflict-free
constexpr int CHUNK_UNIT = 2048;      // rows of a weight-gradient chunk: CHUNK_UNIT x the smallest factor that keeps ...
constexpr int MAX_CHUNKS = 128;       // ... the chunk count at or below this

}  // namespace dplan

namespace dactor {

// The shapes of a net: obs_kind DCOMP_MULTI (one head, a row per (env, UE)) or DCOMP_CENTRAL (U heads, a row per env), U UE slots,
// B stations, hidden width H (a multiple of 32; dcomp_actor.hip's fcnet_shape_check says which shapes are accepted).
struct ActorPlan {
    int32_t multi, hidden;
    int32_t K1, heads, N3;            // inputs, heads, logits of a row
    int32_t mt, Hp, KS2;              // MT of the kernel templates: tiles of 32 hidden units (1, 2, 4 or 8); the padded width; k steps of layers 2 and 3
    int32_t K1p, NT3, NT3v;           // inputs padded to k steps of 16; logit tiles; the same with the shared value's column N3 behind the last head
    int32_t chunks;                   // staging chunks of <= KC inputs layer1 walks
    int32_t XS, lds_per_wave;         // row stride (bf16 elements) of the staged chunk; a wave's LDS slice: the chunk, the logit tile, 16 bytes per row
};

inline ActorPlan actor_plan(int obs_kind, int U, int B, int H)
{
    const bool multi = obs_kind == DCOMP_MULTI;
    const int K1 = multi ? 4 * B + 1 : U * (2 * B + 1), heads = multi ? 1 : U, N3 = heads * (B + 1);
    ActorPlan p;
    p.multi = multi; p.hidden = H; p.K1 = K1; p.heads = heads; p.N3 = N3;
    p.mt = H <= 32 ? 1 : H <= 64 ? 2 : H <= 128 ? 4 : 8;
    p.Hp = 32 * p.mt; p.KS2 = 2 * p.mt;
    p.K1p = (K1 + 15) & ~15; p.NT3 = (N3 + 31) / 32;
    p.NT3v = N3 / 32 + 1;                                    // output N3 = lane N3 % 32 of tile N3 / 32 (a new tile when N3 % 32 == 0)
    p.chunks = (p.K1p + dplan::KC - 1) / dplan::KC;
    p.XS = (p.K1p < dplan::KC ? p.K1p : dplan::KC) + 8;                    // row stride = an odd number of 16-byte slots: 16 rows, 16 slots
    p.lds_per_wave = dplan::TILE * p.XS * 2 + dplan::TILE * dplan::LT * 4 + dplan::TILE * 16;
    return p;
}

DCOMP_PLAN_HD inline int64_t tiles_of(int64_t rows) { return (rows + dplan::TILE - 1) / dplan::TILE; }

// the persistent grid: two workgroups of four waves per CU (two waves per SIMD), a wave per tile up to that
inline int max_blocks_of(int cus) { return (cus > 0 ? cus : 256) * 2; }
inline int launch_blocks(int64_t tiles, int max_blocks)
{
    const int64_t want = (tiles + dplan::WAVES - 1) / dplan::WAVES;
    return (int)(want < max_blocks ? want : max_blocks);
}

}  // namespace dactor

namespace dlearn {

using namespace dactor;

constexpr int NARR = 12;                  // w1 b1 w2 b2 w3 b3 | vw1 vb1 vw2 vb2 wv bv

// a wave's block of dW: MB x NB tiles of 32 x 32 -- 2 x 4 (six operand loads feed eight MFMAs per 16 rows) where the tile counts
// divide, 1 where they do not (the out = 1 tile of a small head, an odd number of input tiles)
DCOMP_PLAN_HD inline int wgrad_mb(int mi_tiles) { return mi_tiles % 2 == 0 ? 2 : 1; }
DCOMP_PLAN_HD inline int wgrad_nb(int ni_tiles) { return ni_tiles % 4 == 0 ? 4 : 1; }

struct LearnerPlan {
    int32_t K1pp, N3p;                                       // inputs and logits padded to tiles of 32
    // the six weight-gradient products dW1 dW2 dW3 | dvW1 dvW2 dwv: padded widths, the block of a wave, its tasks in wgrad_kernel's
    // grid (nmain block tasks from first_task on, then out_p / 32 / nb bias tasks)
    int32_t in_p[6], out_p[6], mb[6], nb[6], nmain[6], first_task[6], ntask;
    // the twelve natural-layout arrays [nin][nout] (a bias: nin = 1) at `off` of the flat arrays
    int32_t nin[NARR], nout[NARR], off[NARR], len[NARR], total;
    // the row stride of the [width][rows] workspaces: whole tiles, + 128 bytes so that a power-of-two batch does not put the 32 rows a
    // wgrad operand load touches into one memory channel
    static int64_t ld_of(int64_t max_rows) { return ((max_rows + 31) & ~(int64_t)31) + 64; }
};

inline LearnerPlan learner_plan(const ActorPlan &a)
{
    LearnerPlan p;
    p.K1pp = (a.K1 + 31) & ~31; p.N3p = 32 * a.NT3;
    const int in_p[6] = {p.K1pp, a.Hp, a.Hp, p.K1pp, a.Hp, a.Hp}, out_p[6] = {a.Hp, a.Hp, p.N3p, a.Hp, a.Hp, 32};
    p.ntask = 0;
    for (int i = 0; i < 6; i++) {
        const int mi_tiles = in_p[i] / 32, ni_tiles = out_p[i] / 32;
        p.in_p[i] = in_p[i]; p.out_p[i] = out_p[i]; p.mb[i] = wgrad_mb(mi_tiles); p.nb[i] = wgrad_nb(ni_tiles);
        p.first_task[i] = p.ntask; p.nmain[i] = (mi_tiles / p.mb[i]) * (ni_tiles / p.nb[i]);
        p.ntask += p.nmain[i] + ni_tiles / p.nb[i];
    }
    const int H = a.hidden, nin[NARR] = {a.K1, 1, H, 1, H, 1, a.K1, 1, H, 1, H, 1}, nout[NARR] = {H, H, H, H, a.N3, a.N3, H, H, H, H, 1, 1};
    p.total = 0;
    for (int i = 0; i < NARR; i++) { p.nin[i] = nin[i]; p.nout[i] = nout[i]; p.off[i] = p.total; p.len[i] = nin[i] * nout[i]; p.total += p.len[i]; }
    return p;
}

// the row split of the weight gradients: a function of the row count alone (on the device too: the grouped kernels split each
// policy's own row count)
struct RowSplit {
    int64_t tiles, rows_pad, mult, chunk_rows;
    int32_t nchunks;
};

DCOMP_PLAN_HD inline RowSplit row_split(int64_t rows)
{
    RowSplit s;
    using dplan::CHUNK_UNIT;
    using dplan::MAX_CHUNKS;
    s.tiles = tiles_of(rows); s.rows_pad = s.tiles * dplan::TILE;
    s.mult = (s.rows_pad + (int64_t)CHUNK_UNIT * MAX_CHUNKS - 1) / ((int64_t)CHUNK_UNIT * MAX_CHUNKS);
    s.chunk_rows = CHUNK_UNIT * s.mult;
    s.nchunks = (int)((s.rows_pad + s.chunk_rows - 1) / s.chunk_rows);
    return s;
}

// The grouped launches (include/dcomp_learner_group.h): the policy is a grid axis of up to DCOMP_GROUP_SLICE policies per launch, and a
// workgroup beyond its own policy's tiles or chunks returns at once.  The tile axis is sized by the slice's largest policy: tiles_of is
// monotonic.  The chunk axis is NOT: row_split(rows).nchunks falls where mult steps up (262 144 rows: 128 chunks, 262 176: 65; 300 000:
// 74, 200 000: 98), so it is sized by the largest chunk count among the slice's policies.
inline int group_chunks(const int64_t *rows, int policies)
{
    int most = 0;
    for (int i = 0; i < policies; i++) {
        if (rows[i] <= 0) continue;                          // sits this call out
        const int c = row_split(rows[i]).nchunks;
        most = c > most ? c : most;
    }
    return most;
}
// x blocks per policy of the grouped learner kernel: the persistent grid shared among the slice's active policies
inline int group_blocks(int64_t max_tiles, int max_blocks, int active)
{
    const int share = max_blocks / (active > 0 ? active : 1);
    return launch_blocks(max_tiles, share > 0 ? share : 1);
}

}  // namespace dlearn

// Introspection for the tests (tests/fcnet_cases.py) and for the binding's own checks (deepcomp_amd.learner.chunk_unit: the unit a
// micro-batch must be a multiple of): the plans of a shape, from the functions above and nothing else.  NOT part of
// the ABI: in no public header, not installed, free to change without an ABI bump.  Makes no HIP call; a shape dcomp_actor_create
// refuses is refused here with the same code.
struct dcomp_fcnet_shape {
    int32_t struct_size;
    int32_t obs_kind, num_ue, num_bs, hidden;
    int64_t rows;                     // the row split of this many rows; 0: none wanted
    int32_t compute_units;            // of the device; 0: the library's fallback
};
struct dcomp_fcnet_desc {
    int32_t struct_size;
    int32_t TILE, WAVES, BLOCK, KC, LT, CHUNK_UNIT, MAX_CHUNKS;
    int32_t max_blocks, grid_tiles;   // max_blocks_of(compute_units), x WAVES: the tiles of one round of the persistent grid
    dactor::ActorPlan actor;
    dlearn::LearnerPlan learner;
    dlearn::RowSplit split;
};
extern "C" int dcomp_fcnet_describe(const dcomp_fcnet_shape *shape, dcomp_fcnet_desc *desc);

#endif
