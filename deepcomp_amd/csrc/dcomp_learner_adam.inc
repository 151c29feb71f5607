// dcomp_learner_adam.inc -- the statements of adam_kernel's body (dcomp_learner.hip), included inside adam_kernel (p: the kernel
// arguments) and adam_group_kernel (p: the view of the policy in blockIdx.y).  Text for the reason dcomp_learner_tiles.inc gives.
// Expects `p` with AParams' member names in scope.
#pragma clang fp contract(off)
static_assert(std::is_same<std::remove_cv_t<decltype(p.total)>, int32_t>::value && sizeof(p.a[0]) == sizeof(ADesc),
              "dcomp_learner_adam.inc is included where p (AParams, or a view with its member names) is in scope");
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= p.total) return;
    float w = p.w[e];
    if (p.adam) {                                                                    // adam_reference: every operation rounded on its own
        const float g = p.g[e];
        const float m = p.m[e] * p.beta1 + g * p.omb1;
        const float v = p.v[e] * p.beta2 + (g * g) * p.omb2;
        const float denom = sqrtf(v) / p.bc2_sqrt + p.eps;
        w = w - p.step_size * (m / denom);
        p.m[e] = m; p.v[e] = v; p.w[e] = w;
    }
    const int ai = find_array(p, e);
    const ADesc d = p.a[ai];
    const int idx = e - d.off;
    if (d.is_bias) {
        d.bias[idx] = w;
        return;
    }
    const int k = idx / d.nout, o = idx - k * d.nout;
    const uint16_t q = bf16_rne(w);
    d.fwd[pack_index(k, o, d.fwd_ks, d.fwd_perm)] = q;
    if (d.bwd) d.bwd[pack_index(o, k, d.bwd_ks, d.bwd_perm)] = q;                     // the other orientation: W^T
