// dcomp_learner_accumulate.inc -- the statements of accumulate_kernel's body (dcomp_learner.hip), included inside accumulate_kernel
// (p: the kernel arguments) and accumulate_group_kernel (p: the view of the policy in blockIdx.y; acc / sums: that policy's slices).
// Text for the reason dcomp_learner_tiles.inc gives.  Expects `p` with AParams' member names, `acc` (float *) and `sums` (double *)
// in scope.
static_assert(std::is_same<std::remove_cv_t<decltype(p.total)>, int32_t>::value && sizeof(p.a[0]) == sizeof(ADesc),
              "dcomp_learner_accumulate.inc is included where p (AParams, or a view with its member names) is in scope");
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < p.total) {
        const int ai = find_array(p, e);
        const ADesc d = p.a[ai];
        const int idx = e - d.off, k = idx / d.nout, o = idx - k * d.nout;
        const size_t stride = d.is_bias ? (size_t)d.out_p : (size_t)d.in_p * d.out_p, at = (size_t)k * d.out_p + o;
        float s = acc[e];
        for (int c = 0; c < p.nchunks; c++) s += d.part[c * stride + at];             // chunk order
        acc[e] = s;
    }
    if (blockIdx.x == 0) {
        __shared__ double sh[256][4];
        const int64_t per = (p.tiles + 255) / 256, lo = threadIdx.x * per, hi = lo + per < p.tiles ? lo + per : p.tiles;
        double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
        for (int64_t t = lo; t < hi; t++) {
            const double *v = p.tile_part + 4 * t;
            s0 += v[0]; s1 += v[1]; s2 += v[2]; s3 += v[3];
        }
        sh[threadIdx.x][0] = s0; sh[threadIdx.x][1] = s1; sh[threadIdx.x][2] = s2; sh[threadIdx.x][3] = s3;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t0 = 0., t1 = 0., t2 = 0., t3 = 0.;
            for (int i = 0; i < 256; i++) { t0 += sh[i][0]; t1 += sh[i][1]; t2 += sh[i][2]; t3 += sh[i][3]; }
            sums[0] += t0; sums[1] += t1; sums[2] += t2; sums[3] += t3; sums[4] += p.count;
        }
    }
