// dcomp_learner_finish.inc -- the statements of finish_kernel's body (dcomp_learner.hip), included inside finish_kernel (p: the kernel
// arguments) and finish_group_kernel (p: the FParams of the policy in blockIdx.y).  Text for the reason dcomp_learner_tiles.inc gives.
// Expects `p` (FParams) in scope.
static_assert(std::is_same<std::remove_cv_t<decltype(p)>, FParams>::value, "dcomp_learner_finish.inc is included where p (FParams) is in scope");
    __shared__ float coef_sh;
    const float scale = accum_scale(p.sums);
    float coef = 1.f;
    if (p.want_norm) {
        if (threadIdx.x == 0) {
            double s = 0.;
            for (int i = 0; i < p.nparts; i++) s += p.norm_part[i];
            const double norm = sqrt(s), c = (double)p.clip / (norm + 1e-6);
            coef_sh = p.clip > 0.f ? (float)(c < 1.0 ? c : 1.0) : 1.f;
            if (blockIdx.x == 0 && p.grad_norm) *p.grad_norm = (float)norm;
        }
        __syncthreads();
        coef = coef_sh;
    }
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < p.total) {
        float g = p.acc[e] * scale;
        if (p.clip > 0.f) g = g * coef;
        p.g[e] = g;
    }
    if (p.stats && blockIdx.x == 0 && threadIdx.x == 0) {
        const double t0 = p.sums[0], t1 = p.sums[1], t2 = p.sums[2], t3 = p.sums[3], count = p.sums[4];
        const double inv = count > 0. ? 1.0 / count : 0.0;
        const float pol = (float)(-t0 * inv), kl = (float)(t1 * inv), ent = (float)(t2 * inv), vfl = (float)(t3 * inv);
        p.stats[0] = pol + p.kl_coeff * kl + p.vf_coeff * vfl - p.ent_coeff * ent;
        p.stats[1] = pol; p.stats[2] = vfl; p.stats[3] = kl; p.stats[4] = ent;
    }
