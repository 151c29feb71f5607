// dcomp_actor.hip -- a trained fcnet actor on the device (include/dcomp.h: dcomp_actor_create / dcomp_actor_actions), its value
// function (dcomp_actor_set_value / dcomp_actor_actions_v) and the advantages of a sample batch (dcomp_gae).
//
// What the reference does with a trained policy (simulation.py:347,375,512-541: trainer.compute_action per env and step) for a
// whole batch in one launch: observation tensor -> two hidden layers -> logits -> categorical draw -> the uint8 action tensor
// dcomp_step takes.  The arithmetic is the specification:
//     x = bf16(obs row);  h1 = bf16(act(x W1 + b1));  h2 = bf16(act(h1 W2 + b2));  logits = h2 W3 + b3
// with bf16 products, f32 accumulation (v_mfma_f32_32x32x16_bf16), bias and activation in f32.
//
// Shape of the kernel.  One WAVEFRONT owns a tile of 32 decision rows and shares nothing with the other waves of its workgroup
// (no workgroup barrier).  Everything is computed transposed, H^T = W^T X^T: the weights are the A operand, the 32 decision rows
// sit on the lanes as the B operand.  The 32 x 32 f32 accumulator of a tile of 32 hidden units then has the hidden unit in its
// 16 registers and the decision row on its lane -- and the next layer sums over exactly that register index, so after bias,
// activation and the bf16 conversion registers 8s ... 8s+7 ARE the B fragment of the next layer's k-step s: the activations never
// leave the registers.  Inside such a step the k order is permuted (element j of lane half h is hidden unit 16s + 8(j>>2) + 4h +
// (j&3)); dcomp_actor_create lays W2 and W3 out in that order, and W1 in the natural order of a fragment read from LDS.
//   - observation rows: read once, coalesced, converted to bf16 into the wave's LDS slice [32][chunk + 8] (chunks of <= 144
//     inputs: a central row of 1 024 inputs needs no more LDS than a multi-agent row, four waves stay under 64 KB); the compact record
//     (dcomp_fragment.h) is expanded on the way in, to the values dcomp_unpack_fragment would have written
//   - weights: packed fragments, 1 KiB per wave-instruction, from L2 (<= 170 KB in all); K and N are padded with zeros in the
//     packed weights, the hidden width to 32 / 64 / 128 / 256 (act(0 + 0) = 0 contributes nothing)
//   - logits: 32 at a time through a [32][33] LDS tile; lane r < 32 walks row r's columns in order -- Gumbel noise, first
//     maximum, online log-sum-exp -- carrying (head, action) across tiles, so heads need not align with anything
//   - rows beyond the batch in the last tile are computed on zeros and never stored
//
// The value function (dcomp_actor_set_value / dcomp_actor_actions_v) rides in the same launch, in instantiations of their own (VF):
//   - VF = 1, a trunk of its own (vf_share_layers=False): a SECOND SWEEP over the wave's tile with the value weights -- layer 1's
//     accumulators of both trunks do not fit the register file side by side.  A row that fits one input chunk is still in the
//     wave's LDS slice as bf16 and is not staged again; multi-chunk rows are re-staged (L2-hot).  value_out is one more 32-wide
//     output tile with a single live column
//   - VF = 2, value_out on the actor's h2: one more column behind the last head in the packed W3; the row walk never sees it
//   - the value-only call (action == NULL) runs the value sweep alone (VF = 1) / the one output tile that holds the column (VF = 2)
// VF = 0 is what dcomp_actor_actions launches, with or without a value function attached.
//
// One policy per UE slot (include/dcomp_policy_set.h: D3-CoMP) is the same kernel with another tile map, instantiations of their own
// (PER, see actor_kernel): a tile is 32 envs of one slot, its trunks come from the set's device table of pointers into the members'
// images.  The set's entry points follow dcomp_actor_actions_v and share actor_launch.  One policy per UE ID
// (include/dcomp_policy_set_uid.h), for envs whose UE list shifts, is a third tile map: a tile is 32 envs of one policy, and its
// prologue finds the slot of the policy's UE in each env from the env's uid words.
//
// This file has the actor's own: the staging of observation rows and compact records (the fetch it hands to layer1), the ring that
// streams the weights of layers 2 and 3, the row walk with its draws, and the entry points.  The pieces the learner's kernel runs
// too -- layer 1, the hidden fragments, the logit tile, the log-sum-exp step -- the fragment layout, the net description (Net) and
// the host helpers are in dcomp_actor_impl.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#define DCOMP_BUILDING_LIBRARY 1
#include "../../include/dcomp.h"
#include "../../include/dcomp_policy_set.h"
#include "../../include/dcomp_policy_set_uid.h"
#include "dcomp_actor_impl.h"       // the forward-pass helpers, the fragment layout, Net and struct dcomp_actor, fail / HIP_TRY: shared with dcomp_learner.hip

namespace dactor {

constexpr uint32_t DRAW_TAG = 0x00AC7012u;

struct Params {
    const void *obs;
    uint8_t *action;
    float *logits, *logp, *vf;
    Net net;                          // the handle's; VF = 2: pi.w3 / pi.b3, NT3 and N3 are the output tiles this call walks (actor_launch)
    int64_t rows, tiles, row_base;
    int32_t num_active, compact, sample;
    uint32_t step, seed_lo, seed_hi;
    int32_t vcol, policy;             // VF = 2: the value's column of the packed W3; policy = 0: the value-only call
    // PER (a policy set, include/dcomp_policy_set.h) only, behind everything the other instantiations read:
    const Trunk *table;               // [U][2]: slot u's policy trunk, value trunk -- pointers into its member's images
    int32_t envs;                     // E; tiles = ceil(E / 32) * U
    // BY_ID (a set keyed by UE id, include/dcomp_policy_set_uid.h) only: table is [P][2] in member order, tiles = ceil(E / 32) * P
    int32_t members;                  // P
    const uint16_t *uid;              // [E][U]: the env's uid words, the layout obs stands in
};

// the tile maps of actor_kernel (its PER parameter): one policy for every row; one per UE slot (include/dcomp_policy_set.h); one per UE id
// (include/dcomp_policy_set_uid.h)
constexpr int SHARED = 0, BY_SLOT = 1, BY_ID = 2;
constexpr uint32_t ABSENT = 0xFFFFFFFFu;      // BY_ID: the entry of a tile row whose env does not list the tile's UE

// entry i (wave-uniform) of a policy set's table.  The table is written once, before any launch: read through the constant address
// space the twelve pointers are scalar loads into SGPRs, like the kernel arguments select_trunk picks from.
__device__ __forceinline__ Trunk slot_trunk(const Trunk *table, int i)
{
    typedef const uint64_t __attribute__((address_space(4))) *cptr;
    cptr q = (cptr)(uintptr_t)(table + i);
    Trunk t;
    t.w1 = reinterpret_cast<const uint4 *>(q[0]); t.w2 = reinterpret_cast<const uint4 *>(q[1]); t.w3 = reinterpret_cast<const uint4 *>(q[2]);
    t.b1 = reinterpret_cast<const float *>(q[3]); t.b2 = reinterpret_cast<const float *>(q[4]); t.b3 = reinterpret_cast<const float *>(q[5]);
    return t;
}
static_assert(sizeof(Trunk) == 6 * sizeof(uint64_t), "slot_trunk reads a Trunk as six 64-bit words");

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}


// MT = hidden width / 32 (padded: 1, 2, 4 or 8); VF: 0 = no value, 1 = a value trunk of its own, 2 = value_out on the actor's h2
// PER = BY_SLOT: one policy per UE slot.  A tile is 32 ENVS of one slot, tile id = env group * U + slot; lane r's decision row is
// (32 g + r) U + slot, the address the shared launch has it at, and both sweeps' trunks come from the slot's table entry.
// (Env-major: the U tiles of an env group run together, so their strided row reads and 1- and 4-byte stores meet in the same cache
// lines while those are in L2.  Slot-major keeps one or two members' weights in flight instead of U and measured 1-14 % SLOWER,
// profiles/r12_policy_set.txt: the weights are at most 340 KB per member and stay cache-resident either way.)  A row is one column of the B operand and depends on
// no tile-mate, so its results are those of the shared launch with the same weights, bit for bit.
// PER = BY_ID: one policy per UE ID, on envs whose UE list shifts.  A tile is 32 envs of one POLICY, tile id = env group * P + policy
// (env-major, as above).  Its prologue finds the slot at which the policy's UE stands in each of its envs: the 64 lanes read the
// envs' uid rows (32 U contiguous 16-bit words, L2-resident across the P tiles of the group), the lane that meets id == policy + 1
// leaves the slot in ri[row][3], preset to ABSENT.  Lane r's decision row is then (32 g + r) U + that slot -- or none: such a row is
// computed on zeros and nothing is stored for it, like the rows beyond the batch; a tile without any returns after the scan.  The
// tiles of policy 0 write, while they scan, the zeros of the slots no tile owns: dead ones and ids beyond P.  Every index comes
// from a position inside the env's own row, whatever the words hold.
template <int MT, bool RELU, int VF, int PER = SHARED>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void actor_kernel(const Params p)
{
    extern __shared__ uint4 lds4[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const uint32_t lane16 = (uint32_t)lane * 16u;
    const Net &n = p.net;
    unsigned char *base = reinterpret_cast<unsigned char *>(lds4) + (size_t)wave * n.lds_per_wave;
    __bf16 *xs = reinterpret_cast<__bf16 *>(base);                                   // [32][XS] bf16: the chunk of the tile's rows
    float *lt = reinterpret_cast<float *>(base + (size_t)TILE * n.XS * 2);           // [32][LT] f32: 32 logits of every row
    uint32_t *ri = reinterpret_cast<uint32_t *>(lt + TILE * LT);                     // [32][4]: compact record of row r: word offset lo, hi | listed | UE slot
    const int XS = n.XS, K1 = n.K1, B = n.B, U = n.U, NA = B + 1;
    constexpr int KS2 = 2 * MT;                                  // k steps of layers 2 and 3
    constexpr int D = KS2 < 8 ? KS2 : 8;                         // weight fragments in flight (32 registers at most)
    constexpr int Q2 = MT * KS2;                                 // MFMAs of layer 2
    const int CW = ue_words(B);
    const uint32_t *cwords = reinterpret_cast<const uint32_t *>(p.obs);
    const float *rowsf = reinterpret_cast<const float *>(p.obs);

    for (int64_t tile = (int64_t)blockIdx.x * WAVES + wave; tile < p.tiles; tile += (int64_t)gridDim.x * WAVES) {
        int pslot = 0, env0 = 0;                                                     // PER: the tile's UE slot (BY_ID: policy) and first env, wave-uniform
        if constexpr (PER == BY_SLOT) {
            const uint32_t id = __builtin_amdgcn_readfirstlane((uint32_t)tile);      // (tiles <= rows / 32 + U < 2^32)
            pslot = (int)(id % (uint32_t)U);
            env0 = TILE * (int)(id / (uint32_t)U);
        }
        if constexpr (PER == BY_ID) {                                                // (P may exceed U: the tile count need not fit 32 bits)
            const int64_t g = tile / p.members;
            pslot = __builtin_amdgcn_readfirstlane((int)(tile - g * p.members));
            env0 = __builtin_amdgcn_readfirstlane(TILE * (int)g);
        }
        const int64_t row0 = tile * TILE;
        const int nrow = PER ? (p.envs - env0 < TILE ? p.envs - env0 : TILE) : (int)(p.rows - row0 < TILE ? p.rows - row0 : TILE);
        if constexpr (PER == BY_ID) {
            if (lane < TILE) ri[lane * 4 + 3] = ABSENT;
            wave_fence();
            const uint16_t *words = p.uid + (size_t)env0 * U;
            const int nw = nrow * U;
            bool found = false;
            for (int i = lane; i < nw; i += 64) {
                const uint32_t id = words[i] & 0x7FFFu;
                const int rr = (int)((uint32_t)i / (uint32_t)U), s = i - rr * U;
                if (id == (uint32_t)pslot + 1u) { ri[rr * 4 + 3] = (uint32_t)s; found = true; }
                if (pslot == 0 && id - 1u >= (uint32_t)p.members) {                  // dead, or a UE beyond the set: no tile owns the row
                    const size_t at = (size_t)(env0 + rr) * U + s;
                    if (p.action) p.action[at] = 0;
                    if (p.logp) p.logp[at] = 0.f;
                    if (p.logits)
                        for (int c = 0; c < n.N3; c++) p.logits[at * n.N3 + c] = 0.f;
                    if (VF != 0) p.vf[at] = 0.f;
                }
            }
            wave_fence();
            if (!__any(found)) continue;                                             // no env of the tile lists the policy's UE
        }
        auto present = [&](int rr) -> bool {                                         // the tile's row rr is a decision row
            if constexpr (PER == BY_ID) return rr < nrow && ri[rr * 4 + 3] != ABSENT;
            else return rr < nrow;
        };
        auto row_of = [&](int rr) -> int64_t {                                       // the decision row of the tile's row rr (BY_ID: where present)
            if constexpr (PER == BY_ID) return (int64_t)(env0 + rr) * U + (int)ri[rr * 4 + 3];
            else if constexpr (PER == BY_SLOT) return (int64_t)(env0 + rr) * U + pslot;
            else return row0 + rr;
        };
        int64_t myrow;                                                               // the decision row on this lane
        bool have;
        if constexpr (PER == BY_ID) {
            have = present(r);
            myrow = have ? row_of(r) : 0;
        } else {
            myrow = row_of(r);
            have = r < nrow;
        }
        int slot = PER == BY_SLOT ? pslot : 0;                                       // multi-agent: the row's UE slot
        if (PER == SHARED && n.multi && have) slot = (int)(myrow % U);
        if (PER == BY_ID && have) slot = (int)ri[r * 4 + 3];
        if (p.compact) {
            if (lane < TILE) {
                uint32_t lo = 0, hi = 0, listed = 0;
                if (have) {
                    const int64_t env = PER ? (int64_t)(env0 + r) : myrow / U;
                    const uint64_t off = (uint64_t)env * (uint64_t)env_words(U, B) + (uint64_t)slot * CW;
                    lo = (uint32_t)off; hi = (uint32_t)(off >> 32); listed = compact_listed(cwords, off, B);
                }
                ri[lane * 4 + 0] = lo; ri[lane * 4 + 1] = hi; ri[lane * 4 + 2] = listed;
                ri[lane * 4 + 3] = PER == BY_ID && !have ? ABSENT : (uint32_t)slot;
            }
            wave_fence();
        }

        // VF = 1: sweep 0 is the policy, sweep 1 the value trunk (alone in the value-only call); otherwise one sweep
#pragma nounroll
        for (int sweep = (VF == 1 && !p.policy) ? 1 : 0; sweep < (VF == 1 ? 2 : 1); sweep++) {
        const bool val = VF == 1 && sweep != 0;
        const Trunk t = PER ? slot_trunk(p.table, 2 * pslot + (val ? 1 : 0)) : select_trunk(n, val);
        const int NT3 = val ? 1 : n.NT3, N3 = val ? 0 : n.N3;                        // (the value trunk has no logits to walk or store)
        const int vcol = VF == 0 ? -1 : VF == 1 ? (val ? 0 : -1) : p.vcol;
        const bool staged = val && p.policy && n.K1p <= KC;                          // the policy sweep left the bf16 rows in LDS

        // ---- layer 1: acc[m] = W1^T (units 32m ...) x X^T, the inputs in chunks through LDS
        f32x16 acc[MT];
        layer1<MT>(acc, t.w1, n.K1p, xs, XS, lane, lane16, staged,
                   [&](int rr, int k) {
                       float v = 0.f;
                       if (present(rr) && k < K1) {
                           if (!p.compact) {
                               v = rowsf[(size_t)row_of(rr) * K1 + k];
                           } else {
                               const uint64_t off = (uint64_t)ri[rr * 4] | ((uint64_t)ri[rr * 4 + 1] << 32);
                               v = compact_input(cwords, off, ri + rr * 4 + 2, k, B, U, CW);
                           }
                       }
                       return v;
                   },
                   [](int, int) {});

        // ---- h1 = bf16(act(. + b1)) as the B fragments of layer 2 (whose first weights are on their way meanwhile)
        // The weights of layers 2 and 3 come through a ring of D fragments, D MFMAs ahead of their use: fragment q is loaded into
        // slot q % D right after the MFMA that read the slot.  (The scheduling barriers pin that order: left alone the compiler
        // hoists every load of a layer to its top -- 512 registers and spills.)
        uint4 ring[D];
#pragma unroll
        for (int i = 0; i < D; i++) ring[i] = load_frag(t.w2, i, lane16);
        bf16x8 h1[MT][2];
        hidden_fragments<MT, RELU>(acc, t.b1, h, h1);

        // ---- layer 2, one tile of 32 units at a time
        bf16x8 h2[MT][2];
        {
#pragma unroll
            for (int m = 0; m < MT; m++) {
                f32x16 a2;
#pragma unroll
                for (int e = 0; e < 16; e++) a2[e] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS2; ks++) {
                    const int q = m * KS2 + ks;
                    a2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(ring[q % D]), h1[ks >> 1][ks & 1], a2, 0, 0, 0);
                    ring[q % D] = q + D < Q2 ? load_frag(t.w2, q + D, lane16) : load_frag(t.w3, q + D - Q2, lane16);   // behind layer 2: layer 3's first
                    __builtin_amdgcn_sched_barrier(0);
                }
                h2[m][0] = next_fragment<RELU>(a2, 0, t.b2 + 32 * m + 4 * h);
                h2[m][1] = next_fragment<RELU>(a2, 1, t.b2 + 32 * m + 4 * h);
                asm volatile("" : "+v"(h2[m][0]), "+v"(h2[m][1]));       // converted HERE: sunk towards layer 3, the 16 raw floats stay live instead of 8 registers
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // ---- layer 3 and the choice, 32 logits of every row at a time
        int hd = 0, a = 0, best_a = 0;                           // the walk's state: head, action within it
        float best_y = -INFINITY, best_l = 0.f, first_l = 0.f, mx = -INFINITY, sm = 0.f;
        uint32_t rnd[4] = {0u, 0u, 0u, 0u};
        const uint32_t grow = (uint32_t)(p.row_base + myrow);
        for (int nt = 0; nt < NT3; nt++) {
            f32x16 a3;
#pragma unroll
            for (int i = 0; i < 16; i++) a3[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS2; ks++) {
                a3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(ring[ks % D]), h2[ks >> 1][ks & 1], a3, 0, 0, 0);      // (Q2 and KS2 are multiples of D)
                const int f = nt * KS2 + ks + D;
                ring[ks % D] = load_frag(t.w3, f < NT3 * KS2 ? f : 0, lane16);                // (behind the last: any valid one)
                __builtin_amdgcn_sched_barrier(0);
            }
            // (put_logit_tile, written out: through the shared function the allocator reloads spilled scalars inside layer 1's staging
            // loop and the compact-record loop runs 0.7 % slower, profiles/r10_fcnet_refactor.txt)
            const float *bias = t.b3 + 32 * nt + 4 * h;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const float4 bv = *reinterpret_cast<const float4 *>(bias + 8 * g);
                float *d = lt + r * LT + 8 * g + 4 * h;
                d[0] = a3[4 * g + 0] + bv.x; d[1] = a3[4 * g + 1] + bv.y; d[2] = a3[4 * g + 2] + bv.z; d[3] = a3[4 * g + 3] + bv.w;
            }
            wave_fence();
            const int ncol = N3 - 32 * nt < 32 ? N3 - 32 * nt : 32;                          // (<= 0: a tile that holds the value's column only)
            if (lane < TILE && have) {
                for (int c = 0; c < ncol; c++) {
                    const float x = lt[r * LT + c];
                    float y = x;
                    if (p.sample) {
                        if ((a & 3) == 0) philox4x32_10(grow, ((uint32_t)hd << 16) | (uint32_t)(a >> 2), p.step, DRAW_TAG, p.seed_lo, p.seed_hi, rnd);
                        const uint32_t w = (a & 3) == 0 ? rnd[0] : (a & 3) == 1 ? rnd[1] : (a & 3) == 2 ? rnd[2] : rnd[3];
                        // u in (0, 1): the f32 sum rounds the top values to 1.0, where the Gumbel draw would be infinite
                        const float u = fminf(((float)(w >> 8) + 0.5f) * 5.9604644775390625e-8f, 0.99999994f);
                        y = x - logf(-logf(u));
                    }
                    if (a == 0) first_l = x;
                    if (y > best_y) { best_y = y; best_a = a; best_l = x; }       // strict: the FIRST maximum
                    if (p.logp) {
                        float e1, e2;
                        lse_push(x, mx, sm, e1, e2);
                    }
                    if (++a == NA) {
                        const bool off = (n.multi ? slot : hd) >= p.num_active;    // unlisted slot / head: action 0
                        const size_t at = (size_t)myrow * n.heads + hd;
                        p.action[at] = (uint8_t)(off ? 0 : best_a);
                        if (p.logp) p.logp[at] = (off ? first_l : best_l) - (mx + logf(sm));
                        a = 0; hd++;
                        best_y = -INFINITY; best_a = 0; mx = -INFINITY; sm = 0.f;
                    }
                }
            }
            if (p.logits) {
                for (int i = lane; i < TILE * 32; i += 64) {
                    const int rr = i >> 5, c = i & 31;
                    if (present(rr) && c < ncol) p.logits[(size_t)row_of(rr) * N3 + 32 * nt + c] = lt[rr * LT + c];
                }
            }
            if (VF != 0) {
                const int vc = vcol - 32 * nt;                                       // the value's column, if this tile holds it
                if (vc >= 0 && vc < 32 && lane < TILE && have) p.vf[myrow] = lt[r * LT + vc];
            }
            wave_fence();
        }
        }
    }
}

typedef void (*kernel_fn)(const Params);
template <int VF, int PER = SHARED> static kernel_fn pick_width(int mt, bool relu)
{
    return pick_shape(mt, relu, [](auto s) -> kernel_fn { return actor_kernel<decltype(s)::MT, decltype(s)::RELU, VF, PER>; });
}
static kernel_fn pick(int mt, bool relu, int vf)
{
    return vf == 0 ? pick_width<0>(mt, relu) : vf == 1 ? pick_width<1>(mt, relu) : pick_width<2>(mt, relu);
}
static kernel_fn pick_set(int mt, bool relu, int vf)             // a policy set: no value, or trunks of their own
{
    return vf == 0 ? pick_width<0, BY_SLOT>(mt, relu) : pick_width<1, BY_SLOT>(mt, relu);
}
static kernel_fn pick_set_uid(int mt, bool relu, int vf)         // a policy set keyed by UE id
{
    return vf == 0 ? pick_width<0, BY_ID>(mt, relu) : pick_width<1, BY_ID>(mt, relu);
}

// RLlib's compute_advantages(use_gae=True) as pinned f32 operations (include/dcomp.h: dcomp_gae): one lane per column walks t
// backwards, every access coalesced across the columns; 16 bytes per (t, r) and nothing to reuse.
struct GaeParams {
    const float *reward, *vf, *last_vf;
    const uint8_t *end;
    float *adv, *target;
    int64_t R;
    int32_t T;
    float gamma, lambda;
};

__global__ __launch_bounds__(256) void gae_kernel(const GaeParams g)
{
    // every operation rounded on its own (what __fmul_rn / __fadd_rn / __fsub_rn promise): written as plain operators under this
    // pragma, because the HIP headers spell those intrinsics as * and + in THEIR contraction mode and -ffp-contract=fast fuses them
#pragma clang fp contract(off)
    const float *__restrict__ reward = g.reward, *__restrict__ vf = g.vf;
    float *__restrict__ adv = g.adv, *__restrict__ target = g.target;
    const float gl = g.gamma * g.lambda;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < g.R; r += (int64_t)gridDim.x * 256) {
        float nv = g.last_vf ? g.last_vf[r] : 0.f, A = 0.f;
#pragma unroll 4
        for (int t = g.T - 1; t >= 0; t--) {
            const size_t i = (size_t)t * (size_t)g.R + (size_t)r;
            const float rw = reward[i], v = vf[i];
            if (g.end && g.end[t]) { nv = 0.f; A = 0.f; }
            const float d = (rw + g.gamma * nv) - v;
            A = d + gl * A;
            adv[i] = A;
            target[i] = A + v;
            nv = v;
        }
    }
}


}  // namespace dactor


// The shapes a net can have: what dcomp_actor_create refuses before it plans, and dcomp_fcnet_describe with it (the same codes and
// texts).  Host only: no HIP call.
static int fcnet_shape_check(const char *fn, int obs_kind, int U, int B, int H)
{
    if (obs_kind != DCOMP_MULTI && obs_kind != DCOMP_CENTRAL) return fail(DCOMP_EINVAL, "%s: obs_kind %d is neither DCOMP_CENTRAL nor DCOMP_MULTI", fn, obs_kind);
    if (U < 1 || B < 1) return fail(DCOMP_EINVAL, "%s: num_ue %d / num_bs %d must be >= 1", fn, U, B);
    if (H < 32 || H % 32) return fail(DCOMP_EINVAL, "%s: hidden %d is not a multiple of 32 >= 32", fn, H);
    if (B > DCOMP_MAX_BS) return fail(DCOMP_EUNSUPPORTED, "%s: num_bs %d > %d", fn, B, DCOMP_MAX_BS);
    if (U > DCOMP_MAX_UE) return fail(DCOMP_EUNSUPPORTED, "%s: num_ue %d > %d", fn, U, DCOMP_MAX_UE);
    if (H > DCOMP_ACTOR_MAX_HIDDEN) return fail(DCOMP_EUNSUPPORTED, "%s: hidden %d > %d", fn, H, DCOMP_ACTOR_MAX_HIDDEN);
    const dactor::ActorPlan pl = dactor::actor_plan(obs_kind, U, B, H);
    if (pl.K1 > DCOMP_ACTOR_MAX_IN) return fail(DCOMP_EUNSUPPORTED, "%s: a central row of %d x %d has %d inputs > %d", fn, U, B, pl.K1, DCOMP_ACTOR_MAX_IN);
    if (pl.N3 > DCOMP_ACTOR_MAX_LOGITS) return fail(DCOMP_EUNSUPPORTED, "%s: a central row of %d x %d has %d logits > %d", fn, U, B, pl.N3, DCOMP_ACTOR_MAX_LOGITS);
    return DCOMP_OK;
}

extern "C" int dcomp_fcnet_describe(const dcomp_fcnet_shape *s, dcomp_fcnet_desc *d)
{
    const char *fn = "dcomp_fcnet_describe";
    if (!s || !d) return fail(DCOMP_EINVAL, "%s: shape and desc must not be NULL", fn);
    if (int rc = check_struct(fn, "dcomp_fcnet_shape", s->struct_size, sizeof(dcomp_fcnet_shape))) return rc;
    if (int rc = check_struct(fn, "dcomp_fcnet_desc", d->struct_size, sizeof(dcomp_fcnet_desc))) return rc;
    if (s->rows < 0 || s->rows > (1ll << 28)) return fail(DCOMP_EINVAL, "%s: rows %lld outside [0, 2^28]", fn, (long long)s->rows);      // (dcomp_learner_create's max_rows)
    if (s->compute_units < 0) return fail(DCOMP_EINVAL, "%s: compute_units %d < 0", fn, s->compute_units);
    if (int rc = fcnet_shape_check(fn, s->obs_kind, s->num_ue, s->num_bs, s->hidden)) return rc;
    memset(d, 0, sizeof(*d));
    d->struct_size = (int32_t)sizeof(*d);
    d->TILE = dplan::TILE; d->WAVES = dplan::WAVES; d->BLOCK = dplan::BLOCK; d->KC = dplan::KC; d->LT = dplan::LT;
    d->CHUNK_UNIT = dplan::CHUNK_UNIT; d->MAX_CHUNKS = dplan::MAX_CHUNKS;
    d->max_blocks = dactor::max_blocks_of(s->compute_units); d->grid_tiles = d->max_blocks * dplan::WAVES;
    d->actor = dactor::actor_plan(s->obs_kind, s->num_ue, s->num_bs, s->hidden);
    d->learner = dlearn::learner_plan(d->actor);
    if (s->rows > 0) d->split = dlearn::row_split(s->rows);
    return DCOMP_OK;
}

extern "C" int dcomp_actor_create(const dcomp_actor_cfg *cfg, dcomp_actor **out)
{
    using namespace dactor;
    const char *fn = "dcomp_actor_create";
    if (out) *out = nullptr;
    if (!cfg || !out) return fail(DCOMP_EINVAL, "%s: cfg and out must not be NULL", fn);
    if (int rc = check_struct(fn, "dcomp_actor_cfg", cfg->struct_size, sizeof(dcomp_actor_cfg))) return rc;
    // host-only validation first: nothing below touches HIP before the arguments are known to be good
    if (int rc = fcnet_shape_check(fn, cfg->obs_kind, cfg->num_ue, cfg->num_bs, cfg->hidden)) return rc;
    if (cfg->activation != DCOMP_ACT_TANH && cfg->activation != DCOMP_ACT_RELU) return fail(DCOMP_EINVAL, "%s: unknown activation %d", fn, cfg->activation);
    if (!cfg->w1 || !cfg->b1 || !cfg->w2 || !cfg->b2 || !cfg->w3 || !cfg->b3) return fail(DCOMP_EINVAL, "%s: a weight or bias pointer is NULL", fn);

    dcomp_actor *a = new dcomp_actor();
    const ActorPlan &pl = a->plan = actor_plan(cfg->obs_kind, cfg->num_ue, cfg->num_bs, cfg->hidden);
    Net &n = a->net;                                         // the kernels' description of the net: the plan's numbers (the trunks: upload_image)
    n.multi = pl.multi; n.U = cfg->num_ue; n.B = cfg->num_bs;
    n.K1 = pl.K1; n.K1p = pl.K1p; n.XS = pl.XS; n.N3 = pl.N3; n.NT3 = pl.NT3; n.heads = pl.heads; n.lds_per_wave = pl.lds_per_wave;
    a->relu = cfg->activation == DCOMP_ACT_RELU;
    const int H = pl.hidden, Hp = pl.Hp;
    std::vector<uint16_t> p1, p2, p3;
    pack(p1, cfg->w1, pl.K1, H, pl.K1p / 16, pl.mt, false);
    pack(p2, cfg->w2, H, H, pl.KS2, pl.mt, true);
    pack(p3, cfg->w3, H, pl.N3, pl.KS2, pl.NT3, true);
    std::vector<float> bias((size_t)2 * Hp + 32 * pl.NT3, 0.f);
    memcpy(bias.data(), cfg->b1, sizeof(float) * H);
    memcpy(bias.data() + Hp, cfg->b2, sizeof(float) * H);
    memcpy(bias.data() + 2 * Hp, cfg->b3, sizeof(float) * pl.N3);

    hipError_t e = hipGetDevice(&a->device);
    int cus = 0;
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, a->device);
    if (e == hipSuccess) e = upload_image(p1, p2, p3, bias, Hp, &a->dev_mem, &n.pi);
    if (e != hipSuccess) {
        delete a;
        return fail(DCOMP_EHIP, "%s: %s", fn, hipGetErrorString(e));
    }
    a->max_blocks = max_blocks_of(cus);
    *out = a;
    return DCOMP_OK;
}

extern "C" int dcomp_actor_destroy(dcomp_actor *a)
{
    if (!a) return DCOMP_OK;
    hipError_t e = hipFree(a->dev_mem);
    if (a->value_mem) {
        const hipError_t e2 = hipFree(a->value_mem);
        if (e == hipSuccess) e = e2;
    }
    delete a;
    return e == hipSuccess ? DCOMP_OK : fail(DCOMP_EHIP, "dcomp_actor_destroy: hipFree failed: %s", hipGetErrorString(e));
}

// a policy set (include/dcomp_policy_set.h): the members and the device table of every slot's two trunks
struct dcomp_policy_set {
    std::vector<dcomp_actor *> members;
    dactor::Trunk *table;             // device [U][2]
    dactor::Trunk *table_id;          // device [P][2], member order (include/dcomp_policy_set_uid.h): behind table, in its allocation
    int32_t value;                  // the members' value form when the table was written: 0 none, 1 a trunk of its own
};

// dcomp_actor_actions (vf_call = false) and dcomp_actor_actions_v: every check on the host first, then ONE launch.
// set: the same for a policy set, a = its first member (the shapes are equal across members).  by_id: the set's launch keyed by UE
// id (include/dcomp_policy_set_uid.h), one entry point for both forms: vf_call = vf != NULL, and its three checks of its own last
static int actor_launch(const char *fn, bool vf_call, dcomp_actor *a, const dcomp_actor_run *r, const void *obs, uint8_t *action, float *vf, void *stream,
                        const dcomp_policy_set *set = nullptr, bool by_id = false, const uint16_t *uid = nullptr)
{
    using namespace dactor;
    if (!a || !r) return fail(DCOMP_EINVAL, "%s: handle and run must not be NULL", fn);
    if (int rc = check_struct(fn, "dcomp_actor_run", r->struct_size, sizeof(dcomp_actor_run))) return rc;
    if (r->obs_format != DCOMP_ACTOR_ROWS && r->obs_format != DCOMP_ACTOR_COMPACT) return fail(DCOMP_EINVAL, "%s: unknown obs_format %d", fn, r->obs_format);
    if (r->obs_format == DCOMP_ACTOR_COMPACT && !a->net.multi)
        return fail(DCOMP_EUNSUPPORTED, "%s: the compact record exists for multi-agent observations only", fn);
    if (by_id) {
        if (!obs) return fail(DCOMP_EINVAL, "%s: obs must not be NULL", fn);
        if (!action && (r->logits || r->logp)) return fail(DCOMP_EINVAL, "%s: action == NULL is the value-only call: run.logits and run.logp must be NULL", fn);
        if (vf && !set->value) return fail(DCOMP_EINVAL, "%s: the handle has no value function (dcomp_actor_set_value)", fn);
    } else if (!vf_call) {
        if (!obs || !action) return fail(DCOMP_EINVAL, "%s: obs and action must not be NULL", fn);
    } else {
        if (!obs) return fail(DCOMP_EINVAL, "%s: obs must not be NULL", fn);
        if (!vf) return fail(DCOMP_EINVAL, "%s: vf must not be NULL (dcomp_actor_actions is the call without a value)", fn);
        if (!action && (r->logits || r->logp)) return fail(DCOMP_EINVAL, "%s: action == NULL is the value-only call: run.logits and run.logp must be NULL", fn);
        if (!(set ? set->value : a->value)) return fail(DCOMP_EINVAL, "%s: the handle has no value function (dcomp_actor_set_value)", fn);
    }
    if (r->num_envs < 1) return fail(DCOMP_EINVAL, "%s: num_envs %d < 1", fn, r->num_envs);
    if (r->num_active < 0 || r->num_active > a->net.U) return fail(DCOMP_EINVAL, "%s: num_active %d outside [0, %d]", fn, r->num_active, a->net.U);
    const int64_t rows = a->net.multi ? (int64_t)r->num_envs * a->net.U : (int64_t)r->num_envs;
    if (r->row_base < 0 || r->row_base + rows > 0x100000000ll)
        return fail(DCOMP_EINVAL, "%s: decision rows %lld ... %lld do not fit the 32-bit draw counter word", fn, (long long)r->row_base,
                     (long long)(r->row_base + rows - 1));
    if (by_id) {
        if (!uid) return fail(DCOMP_EINVAL, "%s: uid must not be NULL", fn);
        if (r->num_active != a->net.U)
            return fail(DCOMP_EINVAL, "%s: num_active %d is not num_ue %d: the uid words say which slots are listed", fn, r->num_active, a->net.U);
        if (!action && !vf) return fail(DCOMP_EINVAL, "%s: action and vf are both NULL: nothing to compute", fn);
    }
    const int mode = vf_call ? (set ? set->value : a->value) : 0;      // (a set: the form its table was written for, 0 or 1)
    Params p;
    memset(&p, 0, sizeof(p));
    p.obs = obs; p.action = action; p.logits = r->logits; p.logp = r->logp; p.vf = vf;
    p.net = a->net;
    const ActorPlan &pl = a->plan;
    p.rows = rows; p.tiles = tiles_of(rows); p.row_base = r->row_base;
    p.num_active = r->num_active; p.compact = r->obs_format == DCOMP_ACTOR_COMPACT; p.sample = r->sample != 0;
    p.step = r->step; p.seed_lo = (uint32_t)r->seed; p.seed_hi = (uint32_t)(r->seed >> 32);
    p.policy = action != nullptr; p.vcol = -1;
    if (mode == 2) {
        const int first = p.policy ? 0 : pl.NT3v - 1;        // value only: the one output tile that holds the value's column, no logits
        p.net.pi.w3 = a->net.vf.w3 + (size_t)first * pl.KS2 * 64; p.net.pi.b3 = a->net.vf.b3 + 32 * first;
        p.net.NT3 = pl.NT3v - first; p.vcol = pl.N3 - 32 * first;
        if (!p.policy) p.net.N3 = 0;
    }
    if (set) {                                               // tiles of 32 envs per UE slot (members are multi, value form 0 or 1)
        p.table = set->table; p.envs = r->num_envs;
        p.tiles = (int64_t)a->net.U * tiles_of(r->num_envs);
    }
    if (by_id) {                                             // tiles of 32 envs per member, the member's trunks, the slot from the uid words
        p.table = set->table_id; p.members = (int32_t)set->members.size(); p.uid = uid;
        p.tiles = (int64_t)p.members * tiles_of(r->num_envs);
    }
    const int grid = launch_blocks(p.tiles, a->max_blocks);
    hipLaunchKernelGGL(by_id ? pick_set_uid(pl.mt, a->relu != 0, mode) : set ? pick_set(pl.mt, a->relu != 0, mode) : pick(pl.mt, a->relu != 0, mode), dim3(grid), dim3(BLOCK), (size_t)pl.lds_per_wave * WAVES, static_cast<hipStream_t>(stream), p);
    HIP_TRY(hipGetLastError());
    return DCOMP_OK;
}

extern "C" int dcomp_actor_actions(dcomp_actor *a, const dcomp_actor_run *r, const void *obs, uint8_t *action, void *stream)
{
    return actor_launch("dcomp_actor_actions", false, a, r, obs, action, nullptr, stream);
}

extern "C" int dcomp_actor_actions_v(dcomp_actor *a, const dcomp_actor_run *r, const void *obs, uint8_t *action, float *vf, void *stream)
{
    return actor_launch("dcomp_actor_actions_v", true, a, r, obs, action, vf, stream);
}

extern "C" int dcomp_policy_set_create(const dcomp_policy_set_cfg *cfg, dcomp_policy_set **out)
{
    using namespace dactor;
    if (out) *out = nullptr;
    // what needs no dereference of a member
    if (!cfg || !out) return fail(DCOMP_EINVAL, "dcomp_policy_set_create: cfg and out must not be NULL");
    if (int rc = check_struct("dcomp_policy_set_create", "dcomp_policy_set_cfg", cfg->struct_size, sizeof(dcomp_policy_set_cfg))) return rc;
    if (!cfg->members) return fail(DCOMP_EINVAL, "dcomp_policy_set_create: members must not be NULL");
    const int P = cfg->num_policies;
    if (P < 1 || P > DCOMP_MAX_UE) return fail(DCOMP_EINVAL, "dcomp_policy_set_create: num_policies %d outside [1, %d]", P, DCOMP_MAX_UE);
    for (int i = 0; i < P; i++)
        if (!cfg->members[i]) return fail(DCOMP_EINVAL, "dcomp_policy_set_create: member %d is NULL", i);
    // the members agree
    const dcomp_actor *f = cfg->members[0];
    for (int i = 1; i < P; i++) {
        const dcomp_actor *m = cfg->members[i];
        const struct { const char *what; int a, b; } same[] = {
            {"obs_kind", f->net.multi, m->net.multi}, {"num_ue", f->net.U, m->net.U}, {"num_bs", f->net.B, m->net.B}, {"hidden", f->plan.hidden, m->plan.hidden},
            {"activation", f->relu, m->relu}, {"device", f->device, m->device}, {"value function", f->value, m->value}};
        for (const auto &c : same)
            if (c.a != c.b) return fail(DCOMP_EINVAL, "dcomp_policy_set_create: member %d differs from member 0 in %s (%d, %d)", i, c.what, c.b, c.a);
    }
    // agreed, but not supported
    if (!f->net.multi) return fail(DCOMP_EUNSUPPORTED, "dcomp_policy_set_create: DCOMP_CENTRAL members: a central policy is one network by construction");
    if (f->value == 2)
        return fail(DCOMP_EUNSUPPORTED, "dcomp_policy_set_create: members with a shared value function (dcomp_actor_value_cfg.shared = 1) are not supported");
    const int U = f->net.U;
    if (cfg->slot_policy)
        for (int u = 0; u < U; u++)
            if (cfg->slot_policy[u] < 0 || cfg->slot_policy[u] >= P)
                return fail(DCOMP_EINVAL, "dcomp_policy_set_create: slot_policy[%d] = %d outside [0, %d)", u, cfg->slot_policy[u], P);

    if (int rc = check_device("dcomp_policy_set_create", "the members live", f->device)) return rc;
    // (without a value function the second entries are NULL; no launch reads them: set->value keeps the value sweep off, and a member
    // that gets a value function later makes every call on the set fail on the host, set_first)
    std::vector<Trunk> host((size_t)2 * U + (size_t)2 * P);
    for (int u = 0; u < U; u++) {
        const dcomp_actor *m = cfg->members[cfg->slot_policy ? cfg->slot_policy[u] : u % P];
        host[2 * u] = m->net.pi; host[2 * u + 1] = m->net.vf;
    }
    for (int i = 0; i < P; i++) {                            // the table of the launch keyed by UE id: member i is the policy of id i + 1
        host[2 * (U + i)] = cfg->members[i]->net.pi; host[2 * (U + i) + 1] = cfg->members[i]->net.vf;
    }
    dcomp_policy_set *s = new dcomp_policy_set();
    s->members.assign(cfg->members, cfg->members + P);
    s->table = nullptr;
    s->value = f->value;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&s->table), host.size() * sizeof(Trunk));
    if (e == hipSuccess) {
        e = hipMemcpy(s->table, host.data(), host.size() * sizeof(Trunk), hipMemcpyHostToDevice);
        if (e != hipSuccess) (void)hipFree(s->table);
    }
    if (e != hipSuccess) {
        delete s;
        return fail(DCOMP_EHIP, "dcomp_policy_set_create: %s", hipGetErrorString(e));
    }
    s->table_id = s->table + (size_t)2 * U;
    *out = s;
    return DCOMP_OK;
}

extern "C" int dcomp_policy_set_destroy(dcomp_policy_set *s)
{
    if (!s) return DCOMP_OK;
    const hipError_t e = hipFree(s->table);
    delete s;
    return e == hipSuccess ? DCOMP_OK : fail(DCOMP_EHIP, "dcomp_policy_set_destroy: hipFree failed: %s", hipGetErrorString(e));
}

// the checks that come before the set is dereferenced (actor_launch repeats them on the first member: the same order as for an actor),
// then the one the set adds: the table holds the trunks the members had at create, so a value function attached to a member since
// (dcomp_actor_set_value works once per handle) is not in it -- refused here, on the host, for every call on the set
static int set_first(const char *fn, dcomp_policy_set *s, const dcomp_actor_run *r, dcomp_actor **first)
{
    if (!s || !r) return fail(DCOMP_EINVAL, "%s: handle and run must not be NULL", fn);
    if (int rc = check_struct(fn, "dcomp_actor_run", r->struct_size, sizeof(dcomp_actor_run))) return rc;
    for (size_t i = 0; i < s->members.size(); i++)
        if (s->members[i]->value != s->value)
            return fail(DCOMP_EINVAL, "%s: member %d got a value function after the set was created (value form %d, the set's %d): attach value "
                        "functions first, then create the set", fn, (int)i, s->members[i]->value, s->value);
    *first = s->members[0];
    return DCOMP_OK;
}

extern "C" int dcomp_policy_set_actions(dcomp_policy_set *s, const dcomp_actor_run *r, const void *obs, uint8_t *action, void *stream)
{
    dcomp_actor *a = nullptr;
    const int rc = set_first("dcomp_policy_set_actions", s, r, &a);
    return rc != DCOMP_OK ? rc : actor_launch("dcomp_policy_set_actions", false, a, r, obs, action, nullptr, stream, s);
}

extern "C" int dcomp_policy_set_actions_v(dcomp_policy_set *s, const dcomp_actor_run *r, const void *obs, uint8_t *action, float *vf, void *stream)
{
    dcomp_actor *a = nullptr;
    const int rc = set_first("dcomp_policy_set_actions_v", s, r, &a);
    return rc != DCOMP_OK ? rc : actor_launch("dcomp_policy_set_actions_v", true, a, r, obs, action, vf, stream, s);
}

extern "C" int dcomp_policy_set_actions_uid(dcomp_policy_set *s, const dcomp_actor_run *r, const void *obs, const uint16_t *uid, uint8_t *action, float *vf,
                                            void *stream)
{
    dcomp_actor *a = nullptr;
    const int rc = set_first("dcomp_policy_set_actions_uid", s, r, &a);
    return rc != DCOMP_OK ? rc : actor_launch("dcomp_policy_set_actions_uid", vf != nullptr, a, r, obs, action, vf, stream, s, true, uid);
}

extern "C" int dcomp_actor_set_value(dcomp_actor *a, const dcomp_actor_value_cfg *cfg)
{
    using namespace dactor;
    if (!a || !cfg) return fail(DCOMP_EINVAL, "dcomp_actor_set_value: handle and cfg must not be NULL");
    if (int rc = check_struct("dcomp_actor_set_value", "dcomp_actor_value_cfg", cfg->struct_size, sizeof(dcomp_actor_value_cfg))) return rc;
    if (cfg->shared != 0 && cfg->shared != 1) return fail(DCOMP_EINVAL, "dcomp_actor_set_value: shared %d is neither 0 nor 1", cfg->shared);
    if (!cfg->wv || !cfg->bv) return fail(DCOMP_EINVAL, "dcomp_actor_set_value: wv or bv is NULL");
    const bool any = cfg->w1 || cfg->b1 || cfg->w2 || cfg->b2, all = cfg->w1 && cfg->b1 && cfg->w2 && cfg->b2;
    if (cfg->shared && any) return fail(DCOMP_EINVAL, "dcomp_actor_set_value: shared = 1 takes value_out only: the trunk pointers w1 ... b2 must be NULL");
    if (!cfg->shared && !all) return fail(DCOMP_EINVAL, "dcomp_actor_set_value: shared = 0 needs the value trunk: a pointer of w1 ... b2 is NULL");
    if (a->value) return fail(DCOMP_EINVAL, "dcomp_actor_set_value: the handle has a value function already (once per handle)");

    if (int rc = check_device("dcomp_actor_set_value", "the handle lives", a->device)) return rc;

    const Net &n = a->net;
    const ActorPlan &pl = a->plan;
    const int H = pl.hidden, Hp = pl.Hp, KS2 = pl.KS2;
    const size_t frag = (size_t)KS2 * 64 * 8;                // bf16 elements of one output tile of a hidden -> out layer
    std::vector<uint16_t> p1, p2, p3;
    std::vector<float> bias;
    if (cfg->shared) {
        // the actor's packed W3 (read back from the handle's device memory) with one more column, NT3v tiles (ActorPlan)
        p3.assign((size_t)pl.NT3v * frag, 0);
        bias.assign((size_t)32 * pl.NT3v, 0.f);
        HIP_TRY(hipMemcpy(p3.data(), n.pi.w3, (size_t)pl.NT3 * frag * 2, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(bias.data(), n.pi.b3, sizeof(float) * 32 * pl.NT3, hipMemcpyDeviceToHost));
        for (int k = 0; k < H; k++) p3[pack_index(k, pl.N3, KS2, true)] = bf16_rne(cfg->wv[k]);
        bias[pl.N3] = cfg->bv[0];
    } else {
        pack(p1, cfg->w1, pl.K1, H, pl.K1p / 16, pl.mt, false);
        pack(p2, cfg->w2, H, H, KS2, pl.mt, true);
        pack(p3, cfg->wv, H, 1, KS2, 1, true);
        bias.assign((size_t)2 * Hp + 32, 0.f);
        memcpy(bias.data(), cfg->b1, sizeof(float) * H);
        memcpy(bias.data() + Hp, cfg->b2, sizeof(float) * H);
        bias[2 * Hp] = cfg->bv[0];
    }
    // shared: no hidden biases in the image, b3 at its start
    void *mem = nullptr;
    const hipError_t e = upload_image(p1, p2, p3, bias, cfg->shared ? 0 : Hp, &mem, &a->net.vf);
    if (e != hipSuccess) return fail(DCOMP_EHIP, "dcomp_actor_set_value: %s", hipGetErrorString(e));
    a->value_mem = mem;
    if (cfg->shared) a->net.vf.b1 = a->net.vf.b2 = nullptr;
    a->value = cfg->shared ? 2 : 1;
    return DCOMP_OK;
}

extern "C" int dcomp_gae(const dcomp_gae_args *g, void *stream)
{
    using namespace dactor;
    if (!g) return fail(DCOMP_EINVAL, "dcomp_gae: args must not be NULL");
    if (int rc = check_struct("dcomp_gae", "dcomp_gae_args", g->struct_size, sizeof(dcomp_gae_args))) return rc;
    if (!g->reward || !g->vf || !g->advantages || !g->value_targets) return fail(DCOMP_EINVAL, "dcomp_gae: reward, vf, advantages and value_targets must not be NULL");
    if (g->num_steps < 1) return fail(DCOMP_EINVAL, "dcomp_gae: num_steps %d < 1", g->num_steps);
    if (g->num_rows < 1) return fail(DCOMP_EINVAL, "dcomp_gae: num_rows %lld < 1", (long long)g->num_rows);
    if (g->num_rows >= (1ll << 40) || (int64_t)g->num_steps * g->num_rows >= (1ll << 40))
        return fail(DCOMP_EINVAL, "dcomp_gae: num_steps x num_rows = %d x %lld is 2^40 elements or more", g->num_steps, (long long)g->num_rows);
    GaeParams k;
    k.reward = g->reward; k.vf = g->vf; k.last_vf = g->last_vf; k.end = g->end; k.adv = g->advantages; k.target = g->value_targets;
    k.R = g->num_rows; k.T = g->num_steps; k.gamma = g->gamma; k.lambda = g->lambda;
    const int64_t want = (g->num_rows + 255) / 256;
    const int grid = (int)(want < (1 << 20) ? want : (1 << 20));          // (beyond: the kernel strides over the columns)
    hipLaunchKernelGGL(gae_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), k);
    HIP_TRY(hipGetLastError());
    return DCOMP_OK;
}
