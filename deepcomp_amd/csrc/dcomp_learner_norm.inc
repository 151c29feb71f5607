// dcomp_learner_norm.inc -- the statements of norm_kernel's body (dcomp_learner.hip), included inside norm_kernel (p: the kernel
// arguments) and norm_group_kernel (p: the FParams of the policy in blockIdx.y).  Text for the reason dcomp_learner_tiles.inc gives.
// Expects `p` (FParams) in scope.
static_assert(std::is_same<std::remove_cv_t<decltype(p)>, FParams>::value, "dcomp_learner_norm.inc is included where p (FParams) is in scope");
    __shared__ double sh[256];
    const float scale = accum_scale(p.sums);
    double s = 0.;
    for (int i = 0; i < NORM_SPAN / 256; i++) {
        const int e = blockIdx.x * NORM_SPAN + i * 256 + threadIdx.x;
        if (e < p.total) {
            const float g = p.acc[e] * scale;
            s += (double)g * (double)g;
        }
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.norm_part[blockIdx.x] = sh[0];
