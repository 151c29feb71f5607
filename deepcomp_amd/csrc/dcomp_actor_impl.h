// dcomp_actor_impl.h -- what dcomp_actor.hip (the actor, its value function) and dcomp_learner.hip (the PPO learner on the same
// handle) share, each piece written once:
//   - the transposed forward pass as far as both kernels run it alike: the MFMA fragment types and helpers, layer 1 through the
//     wave's LDS slice (layer1), the hidden activations as the next layer's B fragments (hidden_fragments), the logit tile
//     (put_logit_tile; actor_kernel has it written out, see there) and the online log-sum-exp step (lse_push).  The streaming of
//     the layer-2 and layer-3 weights is NOT here:
//     the actor's ring across the layer boundary and the learner's group-by-group loads are tuned against different register budgets
//   - the compact record as a kernel's input: its word counts (ue_words, env_words) and the decode of one input of one row
//     (compact_listed, compact_input)
//   - the packed-fragment layout: pack_index() is the permutation and bf16_rne() the rounding, on the host (pack) and on the device
//     (the learner's Adam kernel)
//   - the description of the net (Trunk, Net) that the handle holds and both kernels' arguments embed
//   - host helpers: the failure text (fail, HIP_TRY), the two checks every entry point's prologue makes (check_struct,
//     check_device), the device image of a trunk (upload_image), the width x activation dispatch
// Every shape number of a handle comes from dcomp_fcnet_plan.h (the one statement of the host dispatch); its constants are asserted
// equal to the kernels' below.
// Internal: not installed, not part of the ABI.
#ifndef DCOMP_ACTOR_IMPL_H
#define DCOMP_ACTOR_IMPL_H

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/dcomp.h"
#include "dcomp_fcnet_plan.h"

namespace dcomp { int report(int code, const char *msg); }       // dcomp_api.hip: the thread's dcomp_last_error() text

namespace dactor {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// the kernels' names for the plan's constants (dcomp_fcnet_plan.h, which a host without HIP reads): equal, or this does not compile
constexpr int WAVES = 4, BLOCK = WAVES * 64, TILE = 32;
constexpr int KC = 144;               // inputs staged at a time (a multiple of 16; KC + 8 elements = an odd number of 16-byte slots per row)
constexpr int LT = 33;                // row stride of the logit tile (floats): lanes walk their rows conflict-free
static_assert(WAVES == dplan::WAVES && BLOCK == dplan::BLOCK && TILE == dplan::TILE && KC == dplan::KC && LT == dplan::LT, "dcomp_fcnet_plan.h plans for other constants");

// one trunk: packed bf16 fragments [m tile][k step][lane] x 8 elements, and the biases padded with zeros to the padded widths
struct Trunk {
    const uint4 *w1, *w2, *w3;
    const float *b1, *b2, *b3;
};
// The net of a handle and its shapes.  vf (dcomp_actor_set_value) is, shared = 0, a trunk packed like the policy's with value_out as
// ONE output tile, column 0; shared = 1, vf.w3 / vf.b3 alone: the policy's W3 / b3 with the value's column N3 behind the last head.
struct Net {
    Trunk pi, vf;
    int32_t K1, K1p, XS, N3, NT3, heads, B, U, multi, lds_per_wave;
};

// the trunk of a sweep (field by field: each pointer stays one scalar select between two kernel arguments)
__device__ __forceinline__ Trunk select_trunk(const Net &n, bool val)
{
    return Trunk{val ? n.vf.w1 : n.pi.w1, val ? n.vf.w2 : n.pi.w2, val ? n.vf.w3 : n.pi.w3,
                 val ? n.vf.b1 : n.pi.b1, val ? n.vf.b2 : n.pi.b2, val ? n.vf.b3 : n.pi.b3};
}

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

// the compact record of one env-step (dcomp_fragment.h, whose kernels live in the API object): U x { dr[B] | utility | connection
// mask word(s) } then ues_at_bs[B] | util_at_bs[B]
__host__ __device__ inline int ue_words(int B) { return B + 1 + (B > 32 ? 2 : 1); }
__host__ __device__ inline int env_words(int U, int B) { return U * ue_words(B) + 2 * B; }

// a UE's record at word offset off: listed <=> some dr entry is non-zero
__device__ __forceinline__ uint32_t compact_listed(const uint32_t *cwords, uint64_t off, int B)
{
    uint32_t any = 0;
    for (int b = 0; b < B; b++) any |= cwords[off + b] & 0x7FFFFFFFu;
    return any != 0u;
}

// input k (< 4B + 1) of the observation row of the UE whose record is at word offset off, as dcomp_unpack_fragment would have
// written it: connection bits, dr, the per-env block behind the last UE's record (zeros for an unlisted UE), utility.
// ls: the row's two words listed | UE slot (read only where the per-env block is).  CW = ue_words(B).
__device__ __forceinline__ float compact_input(const uint32_t *cwords, uint64_t off, const uint32_t *ls, int k, int B, int U, int CW)
{
    float v;
    if (k < B) v = (float)((cwords[off + B + 1 + (k >> 5)] >> (k & 31)) & 1u);      // connected
    else if (k < 2 * B) v = __uint_as_float(cwords[off + (k - B)]);                // dr
    else if (k < 4 * B) v = ls[0] ? __uint_as_float(cwords[off + (uint64_t)(U - (int)ls[1]) * CW + (k - 2 * B)]) : 0.f;
    else v = __uint_as_float(cwords[off + B]);                                    // utility
    return v;
}

// Layer 1: acc[m] = W1^T (units 32m ...) x X^T, the K1p inputs in chunks of <= KC through the wave's LDS slice xs [32][XS] bf16.
// fetch(rr, k) -> float is input k of the tile's row rr (0 where there is none); after_stage(k0, kc) runs once per chunk, with
// inputs k0 ... k0 + kc - 1 of the 32 rows in xs.  staged: a single chunk that an earlier sweep left in xs is not fetched again.
template <int MT, class Fetch, class AfterStage>
__device__ __forceinline__ void layer1(f32x16 (&acc)[MT], const uint4 *w1, int K1p, __bf16 *xs, int XS, int lane, uint32_t lane16, bool staged,
                                       Fetch fetch, AfterStage after_stage)
{
    const int r = lane & 31, h = lane >> 5, KS1 = K1p >> 4;
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[m][i] = 0.f;
    uint4 wq1[MT];                                                               // layer 1's weights, one k step ahead
#pragma unroll
    for (int m = 0; m < MT; m++) wq1[m] = load_frag(w1, (size_t)m * KS1, lane16);
    for (int k0 = 0; k0 < K1p; k0 += KC) {
        const int kc = K1p - k0 < KC ? K1p - k0 : KC;                            // a multiple of 16
        const uint32_t magic = (uint32_t)(0x100000000ull / (uint32_t)kc) + 1u;   // f / kc = umulhi(f, magic): f < 2^14, f kc < 2^32
        const int nf = staged ? 0 : TILE * kc;
#pragma unroll 4
        for (int f = lane; f < nf; f += 64) {
            const int rr = (int)__umulhi((uint32_t)f, magic), c = f - rr * kc;
            xs[rr * XS + c] = (__bf16)fetch(rr, k0 + c);
        }
        wave_fence();
        after_stage(k0, kc);
        for (int s = 0; s < (kc >> 4); s++) {
            const bf16x8 b = as_frag(*reinterpret_cast<const uint4 *>(xs + r * XS + 16 * s + 8 * h));
            const int ksn = (k0 >> 4) + s + 1 < KS1 ? (k0 >> 4) + s + 1 : KS1 - 1;          // (the last step re-reads itself)
            uint4 nx[MT];
#pragma unroll
            for (int m = 0; m < MT; m++) nx[m] = load_frag(w1, (size_t)m * KS1 + ksn, lane16);
#pragma unroll
            for (int m = 0; m < MT; m++) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(wq1[m]), b, acc[m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < MT; m++) wq1[m] = nx[m];
        }
        wave_fence();
    }
}

// f = bf16(act(acc + bias)) of a whole layer, as the B fragments of the next layer on lane half h
template <int MT, bool RELU> __device__ __forceinline__ void hidden_fragments(const f32x16 (&acc)[MT], const float *bias, int h, bf16x8 (&f)[MT][2])
{
#pragma unroll
    for (int t = 0; t < MT; t++) {
        f[t][0] = next_fragment<RELU>(acc[t], 0, bias + 32 * t + 4 * h);
        f[t][1] = next_fragment<RELU>(acc[t], 1, bias + 32 * t + 4 * h);
        asm volatile("" : "+v"(f[t][0]), "+v"(f[t][1]));
        __builtin_amdgcn_sched_barrier(0);                       // (tile by tile: 16 registers become 8, not every bias load first)
    }
}

// output tile nt of layer 3 + b3 on lane (r, h) into the [32][LT] logit tile: register i is column (i & 3) + 8 (i >> 2) + 4h of row r
__device__ __forceinline__ void put_logit_tile(const f32x16 &a3, const float *b3, int nt, float *lt, int r, int h)
{
    const float *bias = b3 + 32 * nt + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const float4 bv = *reinterpret_cast<const float4 *>(bias + 8 * g);
        float *d = lt + r * LT + 8 * g + 4 * h;
        d[0] = a3[4 * g + 0] + bv.x; d[1] = a3[4 * g + 1] + bv.y; d[2] = a3[4 * g + 2] + bv.z; d[3] = a3[4 * g + 3] + bv.w;
    }
}

// one step of the online log-sum-exp over a head's logits: the sum rescaled to the new maximum; e1, e2 are the two exponentials,
// for the sums that ride along
__device__ __forceinline__ void lse_push(float x, float &mx, float &sm, float &e1, float &e2)
{
    const float m2 = fmaxf(mx, x);
    e1 = expf(mx - m2); e2 = expf(x - m2);
    sm = sm * e1 + e2;
    mx = m2;
}

__host__ __device__ inline uint16_t bf16_rne(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);      // NaN stays a NaN
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// A fragments of W^T for [tiles of 32 outputs][k steps of 16][lane][8]: lane (r, h) holds output 32 m + r and the inputs
// 16 ks + 8h + j (natural: the B operand is read from LDS) or 16 ks + 8 (j >> 2) + 4h + (j & 3) (permuted: the B operand is the
// previous layer's accumulator).  pack_index is where input k, output o is in such an array.
__host__ __device__ inline size_t pack_index(int k, int o, int ksteps, int permuted)
{
    const int m = o >> 5, r = o & 31, ks = k >> 4, kk = k & 15;
    const int h = permuted ? (kk & 7) >> 2 : kk >> 3, j = permuted ? 4 * (kk >> 3) + (kk & 3) : kk & 7;
    return (((size_t)m * ksteps + ks) * 64 + 32 * h + r) * 8 + j;
}

// w is [in][out] row-major with nin <= 16 ksteps, nout <= 32 mtiles; everything outside [nin][nout] is zero.
static void pack(std::vector<uint16_t> &dst, const float *w, int nin, int nout, int ksteps, int mtiles, bool permuted)
{
    dst.assign((size_t)mtiles * ksteps * 64 * 8, 0);
    for (int k = 0; k < nin; k++)
        for (int o = 0; o < nout; o++) dst[pack_index(k, o, ksteps, permuted)] = bf16_rne(w[(size_t)k * nout + o]);
}

// The instantiation of a kernel template for a handle's padded width (mt = 1, 2, 4 or 8 tiles of 32 units) and activation:
// f(Shape<MT, RELU>()) names it.
template <int MT_, bool RELU_> struct Shape { static constexpr int MT = MT_; static constexpr bool RELU = RELU_; };
template <class F> static auto pick_shape(int mt, bool relu, F f) -> decltype(f(Shape<1, true>()))
{
    switch (mt) {
    case 1: return relu ? f(Shape<1, true>()) : f(Shape<1, false>());
    case 2: return relu ? f(Shape<2, true>()) : f(Shape<2, false>());
    case 4: return relu ? f(Shape<4, true>()) : f(Shape<4, false>());
    default: return relu ? f(Shape<8, true>()) : f(Shape<8, false>());
    }
}

// A trunk's device image: the W1 | W2 | W3 fragments | the biases b1[Hp] b2[Hp] b3, each part at a 256-byte offset of ONE allocation
// (p1 and p2 may be empty, with Hp = 0).  On success *mem is the allocation and t points into it; on failure nothing stays allocated.
static hipError_t upload_image(const std::vector<uint16_t> &p1, const std::vector<uint16_t> &p2, const std::vector<uint16_t> &p3,
                               const std::vector<float> &bias, int Hp, void **mem, Trunk *t)
{
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o1 = 0, o2 = up(o1 + p1.size() * 2), o3 = up(o2 + p2.size() * 2), ob = up(o3 + p3.size() * 2), total = ob + bias.size() * 4;
    std::vector<unsigned char> img(total, 0);
    if (!p1.empty()) memcpy(img.data() + o1, p1.data(), p1.size() * 2);
    if (!p2.empty()) memcpy(img.data() + o2, p2.data(), p2.size() * 2);
    memcpy(img.data() + o3, p3.data(), p3.size() * 2);
    memcpy(img.data() + ob, bias.data(), bias.size() * 4);
    hipError_t e = hipMalloc(mem, total);
    if (e == hipSuccess) {
        e = hipMemcpy(*mem, img.data(), total, hipMemcpyHostToDevice);
        if (e != hipSuccess) (void)hipFree(*mem);
    }
    if (e != hipSuccess) return e;
    unsigned char *d = static_cast<unsigned char *>(*mem);
    t->w1 = reinterpret_cast<const uint4 *>(d + o1); t->w2 = reinterpret_cast<const uint4 *>(d + o2); t->w3 = reinterpret_cast<const uint4 *>(d + o3);
    t->b1 = reinterpret_cast<const float *>(d + ob); t->b2 = t->b1 + Hp; t->b3 = t->b2 + Hp;
    return hipSuccess;
}

}  // namespace dactor

struct dcomp_actor {
    dactor::ActorPlan plan;                                  // every shape number of the handle
    int32_t relu, device, max_blocks;
    dactor::Net net;                                         // (net.multi: the handle's obs_kind is DCOMP_MULTI)
    void *dev_mem;
    // the value function (dcomp_actor_set_value): value = 0 none, 1 a trunk of its own, 2 value_out on the actor's h2
    int32_t value;
    void *value_mem;
};

// an entry point's failure: the text goes to dcomp_last_error(), the code is the return value
static int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return dcomp::report(code, buf);
}
#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return fail(DCOMP_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)


// the two checks of an entry point's prologue.  A struct of the ABI carries its size as its first field:
static int check_struct(const char *fn, const char *name, int32_t got, size_t size)
{
    return got == (int32_t)size ? DCOMP_OK : fail(DCOMP_EABI, "%s: caller's %s has %d bytes, the library's %d", fn, name, got, (int)size);
}
// and a handle is used on the device it was created on (what: "the handle lives")
static int check_device(const char *fn, const char *what, int device)
{
    int dev = -1;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail(DCOMP_EHIP, "%s: %s", fn, hipGetErrorString(e));
    return dev == device ? DCOMP_OK : fail(DCOMP_EINVAL, "%s: %s on device %d, the calling thread's current device is %d", fn, what, device, dev);
}

#endif
