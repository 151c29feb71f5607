// dcomp_actor_impl.h -- what dcomp_actor.hip (the actor, its value function) and dcomp_learner.hip (the PPO learner on the same
// handle) share: the MFMA fragment types and helpers of the transposed forward pass, the host-side fragment packing and the
// handle itself.  Internal: not installed, not part of the ABI.
#ifndef DCOMP_ACTOR_IMPL_H
#define DCOMP_ACTOR_IMPL_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/dcomp.h"

namespace dactor {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int WAVES = 4, BLOCK = WAVES * 64, TILE = 32;
constexpr int KC = 144;               // inputs staged at a time (a multiple of 16; KC + 8 elements = an odd number of 16-byte slots per row)
constexpr int LT = 33;                // row stride of the logit tile (floats): lanes walk their rows conflict-free

// LDS ops of one wave execute in order; this only stops the compiler from moving LDS accesses across it.
__device__ __forceinline__ void wave_fence()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

template <bool RELU> __device__ __forceinline__ float activate(float x)
{
    if (RELU) return fmaxf(x, 0.f);
    // tanh(x) = 1 - 2 / (exp(2x) + 1): exp -> inf gives 1, exp -> 0 gives -1; absolute error ~1e-7, far inside the bf16 rounding of the result
    const float e = __builtin_amdgcn_exp2f(x * 2.885390081777927f);
    return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}

// registers 8s ... 8s+7 of an accumulator tile (+ bias, activation) -> the B fragment of the next layer's k-step s.
// bias points at the tile's first unit + 4 * (lane half): register i holds unit (i & 3) + 8 (i >> 2) + 4h of the tile.
template <bool RELU> __device__ __forceinline__ bf16x8 next_fragment(const f32x16 &acc, int s, const float *bias)
{
    const float4 ba = *reinterpret_cast<const float4 *>(bias + 16 * s), bb = *reinterpret_cast<const float4 *>(bias + 16 * s + 8);
    bf16x8 f;
    f[0] = (__bf16)activate<RELU>(acc[8 * s + 0] + ba.x);
    f[1] = (__bf16)activate<RELU>(acc[8 * s + 1] + ba.y);
    f[2] = (__bf16)activate<RELU>(acc[8 * s + 2] + ba.z);
    f[3] = (__bf16)activate<RELU>(acc[8 * s + 3] + ba.w);
    f[4] = (__bf16)activate<RELU>(acc[8 * s + 4] + bb.x);
    f[5] = (__bf16)activate<RELU>(acc[8 * s + 5] + bb.y);
    f[6] = (__bf16)activate<RELU>(acc[8 * s + 6] + bb.z);
    f[7] = (__bf16)activate<RELU>(acc[8 * s + 7] + bb.w);
    return f;
}

// fragment `idx` (uniform) of a packed weight array for this lane: a uniform base + the lane's 32-bit byte offset.  The offset is
// made opaque at every call: the tile loop's ~150 load addresses are loop-invariant, and hoisted out of it as 64-bit lane
// addresses they were 290 spilled registers.
__device__ __forceinline__ uint4 load_frag(const uint4 *w, size_t idx, uint32_t lane16)
{
    asm volatile("" : "+v"(lane16));
    return *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(w + idx * 64) + lane16);
}

__device__ __forceinline__ bf16x8 as_frag(uint4 v)
{
    union { uint4 u; bf16x8 f; } c;
    c.u = v;
    return c.f;
}

static uint16_t bf16_rne(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);      // NaN stays a NaN
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// A fragments of W^T for [tiles of 32 outputs][k steps of 16][lane][8]: lane (r, h) holds output 32 m + r and the inputs
// 16 ks + 8h + j (natural: the B operand is read from LDS) or 16 ks + 8 (j >> 2) + 4h + (j & 3) (permuted: the B operand is the
// previous layer's accumulator).  w is [in][out] row-major; everything outside [nin][nout] is zero.
static void pack(std::vector<uint16_t> &dst, const float *w, int nin, int nout, int ksteps, int mtiles, bool permuted)
{
    dst.assign((size_t)mtiles * ksteps * 64 * 8, 0);
    for (int m = 0; m < mtiles; m++)
        for (int ks = 0; ks < ksteps; ks++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 8; j++) {
                    const int r = lane & 31, h = lane >> 5, o = 32 * m + r;
                    const int k = 16 * ks + (permuted ? 8 * (j >> 2) + 4 * h + (j & 3) : 8 * h + j);
                    if (k < nin && o < nout) dst[(((size_t)m * ksteps + ks) * 64 + lane) * 8 + j] = bf16_rne(w[(size_t)k * nout + o]);
                }
}

}  // namespace dactor

struct dcomp_actor {
    int32_t kind, U, B, hidden, mt, relu, device;
    int32_t K1, K1p, N3, NT3, heads, XS, lds_per_wave, max_blocks;
    void *dev_mem;
    const uint4 *w1, *w2, *w3;
    const float *b1, *b2, *b3;
    // the value function (dcomp_actor_set_value): value = 0 none, 1 a trunk of its own, 2 value_out on the actor's h2
    int32_t value, NT3v;
    void *value_mem;
    const uint4 *vw1, *vw2, *vw3;                            // value = 2: vw3 / vb3 = the actor's W3 / b3 with the value's column N3 behind the last head
    const float *vb1, *vb2, *vb3;
};

#endif
