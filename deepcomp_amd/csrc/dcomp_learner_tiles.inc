// dcomp_learner_tiles.inc -- the statements of learner_kernel's body (dcomp_learner.hip), included INSIDE a kernel: learner_kernel
// (its arguments are the kernel arguments) and learner_group_kernel (its arguments are put together from the group's table entry
// of the policy in blockIdx.y).  Text, not a function: as an inlined function taking the arguments by reference the existing
// instantiations compiled to other code (tools/isa_stats.py), and they are tuned against 450 of 512 registers.
// Expects in scope: MT, RELU, IDX (constant expressions) and `p` (LParams, or IParams with IDX).  The tile loop walks blockIdx.x /
// gridDim.x.
static_assert(std::is_base_of<LParams, std::remove_cv_t<decltype(p)>>::value && std::is_same<std::remove_cv_t<decltype(IDX)>, bool>::value &&
              std::is_same<std::remove_cv_t<decltype(RELU)>, bool>::value && (MT == 1 || MT == 2 || MT == 4 || MT == 8),
              "dcomp_learner_tiles.inc is included where p (LParams or IParams), MT, RELU and IDX are in scope");
    extern __shared__ uint4 lds4[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const uint32_t lane16 = (uint32_t)lane * 16u;
    const Net &n = p.net;
    unsigned char *base = reinterpret_cast<unsigned char *>(lds4) + (size_t)wave * n.lds_per_wave;
    __bf16 *xs = reinterpret_cast<__bf16 *>(base);                                   // [32][XS] bf16: the chunk of the tile's rows
    float *lt = reinterpret_cast<float *>(base + (size_t)TILE * n.XS * 2);           // [32][LT] f32: 32 logits / dlogits of every row
    // [32]: the row is read and counted.  IDX: [32][4], position r's source row (NO_ROW: nothing is read) | its env | listed | UE slot
    uint32_t *ri = reinterpret_cast<uint32_t *>(lt + TILE * LT);
    const int XS = n.XS, K1 = n.K1, U = n.U, NA = n.B + 1;
    const int B = n.B, CW = ue_words(B);
    const uint32_t *cwords = reinterpret_cast<const uint32_t *>(p.obs);
    constexpr int KS2 = 2 * MT;
    const int64_t ld = p.ld;

    for (int64_t tile = (int64_t)blockIdx.x * WAVES + wave; tile < p.tiles; tile += (int64_t)gridDim.x * WAVES) {
        const int64_t row0 = tile * TILE;
        const int nrow = (int)(p.rows - row0 < TILE ? p.rows - row0 : TILE);
        const int64_t myrow = row0 + r;                                              // the decision row on this lane
        const bool have = r < nrow;
        if constexpr (IDX) {
            // the source row of every position, resolved once per tile; an entry outside the sample batch is never dereferenced
            if (lane < TILE) {
                uint32_t src = NO_ROW, env = 0, listed = 0, slot = 0;
                if (have) {
                    const int64_t s = p.index ? (int64_t)p.index[myrow] : myrow;
                    if (s >= 0 && s < p.source_rows) {
                        src = (uint32_t)s;
                        if (p.compact) {
                            env = src / (uint32_t)U; slot = src - env * (uint32_t)U;
                            listed = compact_listed(cwords, (uint64_t)env * (uint64_t)env_words(U, B) + (uint64_t)slot * CW, B);
                        }
                    }
                }
                ri[lane * 4 + 0] = src; ri[lane * 4 + 1] = env; ri[lane * 4 + 2] = listed; ri[lane * 4 + 3] = slot;
            }
            wave_fence();
        }
        // a row beyond the batch, a multi-agent row of an unlisted slot, or (IDX) a position whose index entry is outside the sample
        // batch: computed on zeros, every delta zero, nothing of it read
        const bool live = IDX ? have && ri[r * 4] != NO_ROW : have && !(n.multi && (int)(myrow % U) >= p.num_active);
        const bool walker = lane < TILE && live;
        const uint32_t voff = (uint32_t)(2 * ((uint64_t)myrow + (uint64_t)(4 * h) * (uint64_t)ld));      // store_frags: this lane's column
        if constexpr (!IDX) {
            if (lane < TILE) ri[lane] = live ? 1u : 0u;
            wave_fence();
        }

        float s_surr = 0.f, s_kl = 0.f, s_ent = 0.f, s_vfl = 0.f;                     // this row's terms (lanes < 32)
        float c_lp = 0.f;                                                            // d(-surrogate) / d(logp)

#pragma nounroll
        for (int sweep = 0; sweep < 2; sweep++) {
        const bool val = sweep != 0;
        const Trunk t = select_trunk(n, val);
        const uint4 *w2b = val ? p.vw2b : p.w2b, *w3b = val ? p.vw3b : p.w3b;
        __bf16 *H1 = val ? p.VH1 : p.H1, *H2 = val ? p.VH2 : p.H2, *D1 = val ? p.VD1 : p.D1, *D2 = val ? p.VD2 : p.D2, *D3 = val ? p.VD3 : p.D3;
        const int NT3 = val ? 1 : n.NT3, N3 = val ? 1 : n.N3;
        const bool staged = val && n.K1p <= KC;                                      // the policy sweep left the bf16 rows in LDS

        // ---- layer 1, with x as bf16 [input][rows] on the way for dW1 of both trunks
        f32x16 acc[MT];
        layer1<MT>(acc, t.w1, n.K1p, xs, XS, lane, lane16, staged,
                   [&](int rr, int k) {
                       if constexpr (IDX) {                                          // at the source row: a float row or a compact record
                           const uint32_t s = ri[rr * 4];
                           float v = 0.f;
                           if (s != NO_ROW && k < K1) {
                               if (!p.compact) v = p.obs[(size_t)s * K1 + k];
                               else v = compact_input(cwords, (uint64_t)ri[rr * 4 + 1] * (uint64_t)env_words(U, B) + (uint64_t)ri[rr * 4 + 3] * CW,
                                                      ri + rr * 4 + 2, k, B, U, CW);
                           }
                           return v;
                       } else {
                           return ri[rr] && k < K1 ? p.obs[(size_t)(row0 + rr) * K1 + k] : 0.f;
                       }
                   },
                   [&](int k0, int kc) {
                       if (!val && !p.fwd_only) {
                           for (int i = lane; i < kc * TILE; i += 64) {
                               const int c = i >> 5, rr = i & 31;
                               p.X[(size_t)(k0 + c) * (size_t)ld + (size_t)(row0 + rr)] = xs[rr * XS + c];
                           }
                       }
                   });

        bf16x8 h1[MT][2];
        hidden_fragments<MT, RELU>(acc, t.b1, h, h1);
        if (!p.fwd_only) store_frags<MT>(H1, ld, voff, h1);

        // ---- layer 2
        bf16x8 h2[MT][2];
#pragma unroll
        for (int m = 0; m < MT; m++) {
            const f32x16 a2 = tile_dot<MT>(t.w2, (size_t)m * KS2, h1, lane16);
            h2[m][0] = next_fragment<RELU>(a2, 0, t.b2 + 32 * m + 4 * h);
            h2[m][1] = next_fragment<RELU>(a2, 1, t.b2 + 32 * m + 4 * h);
            asm volatile("" : "+v"(h2[m][0]), "+v"(h2[m][1]));
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!p.fwd_only) store_frags<MT>(H2, ld, voff, h2);

        // ---- layer 3, first walk: the log-sum-exp of every head (new and old logits), logp of the given action, the entropy
        float logp_sum = 0.f, oldlp_sum = 0.f, ent_sum = 0.f;
        {
            int hd = 0, a = 0, act = 0;
            float xa = 0.f, mx = -INFINITY, sm = 0.f, tn = 0.f, mo = -INFINITY, so = 0.f;
            for (int nt = 0; nt < NT3; nt++) {
                put_logit_tile(tile_dot<MT>(t.w3, (size_t)nt * KS2, h2, lane16), t.b3, nt, lt, r, h);
                wave_fence();
                if (!val && walker && p.actions) {
                    const int ncol = N3 - 32 * nt < 32 ? N3 - 32 * nt : 32;
                    for (int c = 0; c < ncol; c++) {
                        const float x = lt[r * LT + c];
                        if (a == 0) act = p.actions[source_row<IDX>(ri, r, myrow) * n.heads + hd];
                        if (a == act) xa = x;
                        float e1, e2;
                        lse_push(x, mx, sm, e1, e2);
                        tn = tn * e1 + x * e2;
                        if (p.old_logits) lse_push(p.old_logits[source_row<IDX>(ri, r, myrow) * n.N3 + 32 * nt + c], mo, so, e1, e2);
                        if (++a == NA) {
                            const size_t at = (size_t)myrow * n.heads + hd;
                            const float lse = mx + logf(sm), lp = xa - lse, eh = lse - tn / sm;
                            if (p.o_logp) p.o_logp[at] = lp;
                            if (n.multi || hd < p.num_active) {
                                logp_sum += lp; ent_sum += eh;
                                if (p.old_logp) oldlp_sum += p.old_logp[IDX ? source_row<IDX>(ri, r, myrow) * n.heads + hd : at];
                            }
                            if (!p.fwd_only) p.headws[at] = make_float4(lse, mo + logf(so), eh, 0.f);
                            a = 0; hd++; xa = 0.f;
                            mx = -INFINITY; sm = 0.f; tn = 0.f; mo = -INFINITY; so = 0.f;
                        }
                    }
                }
                wave_fence();
            }
        }
        if (!val) {
            if (walker && p.o_ent) p.o_ent[myrow] = ent_sum;
            s_ent = walker ? ent_sum : 0.f;
            if (!p.fwd_only && !p.upstream && walker) {
                const float adv = p.adv[source_row<IDX>(ri, r, myrow)], ratio = expf(logp_sum - oldlp_sum);
                const float s1 = adv * ratio, s2 = adv * fminf(fmaxf(ratio, 1.f - p.clip), 1.f + p.clip);
                s_surr = fminf(s1, s2);
                c_lp = s1 <= s2 ? -s1 : 0.f;                                          // d(-min) / d(logp): d(adv ratio) / d(logp) = adv ratio
                if (p.o_ratio) p.o_ratio[myrow] = ratio;
            }
            if constexpr (IDX) {
                if (lane < TILE && have && !live) {                                  // nothing was read: its outputs are zeros
                    if (p.actions && p.o_logp)
                        for (int hd = 0; hd < n.heads; hd++) p.o_logp[(size_t)myrow * n.heads + hd] = 0.f;
                    if (p.o_ent) p.o_ent[myrow] = 0.f;
                    if (!p.fwd_only && !p.upstream) {
                        if (p.o_ratio) p.o_ratio[myrow] = 0.f;
                        if (p.o_kl) p.o_kl[myrow] = 0.f;
                    }
                }
            }
        } else if (lane < TILE && have && p.o_vf) {
            p.o_vf[myrow] = !IDX || live ? lt[r * LT] : 0.f;                         // (the tile of the value sweep is still in LDS)
        }
        if (p.fwd_only) continue;

        // ---- dlogits tile by tile into the LDS tile, and dH2^T = W3 dlogits^T
        f32x16 dh[MT];
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int i = 0; i < 16; i++) dh[m][i] = 0.f;
        {
            int hd = 0, a = 0, act = 0;
            float4 hw = make_float4(0.f, 0.f, 0.f, 0.f);
            float kl_sum = 0.f;
            for (int nt = 0; nt < NT3; nt++) {
                const int ncol = N3 - 32 * nt < 32 ? N3 - 32 * nt : 32;
                if (val) {
                    // the value's one column: d(vf_loss_coeff max((v - vt)^2, (old_v + clip(v - old_v) - vt)^2)) / dv
                    if (lane < TILE) {
                        float dv = 0.f;
                        if (walker) {
                            if (p.upstream) dv = p.up_dvalue[source_row<IDX>(ri, r, myrow)];
                            else {
                                const float v = lt[r * LT], vt = p.vtarg[source_row<IDX>(ri, r, myrow)], ov = p.old_vf[source_row<IDX>(ri, r, myrow)];
                                const float d1 = v - vt, dc = fminf(fmaxf(v - ov, -p.vf_clip), p.vf_clip), d2 = (ov + dc) - vt;
                                const float l1 = d1 * d1, l2 = d2 * d2;
                                s_vfl = fmaxf(l1, l2);
                                dv = p.vf_coeff * (l1 >= l2 ? 2.f * d1 : (fabsf(v - ov) < p.vf_clip ? 2.f * d2 : 0.f));
                            }
                        }
                        for (int c = 1; c < 32; c++) lt[r * LT + c] = 0.f;
                        lt[r * LT] = dv;
                    }
                } else if (p.upstream) {
                    for (int i = lane; i < TILE * 32; i += 64) {
                        const int rr = i >> 5, c = i & 31;
                        if constexpr (IDX) lt[rr * LT + c] = ri[rr * 4] != NO_ROW && c < ncol ? p.up_dlogits[(size_t)ri[rr * 4] * n.N3 + 32 * nt + c] : 0.f;
                        else lt[rr * LT + c] = ri[rr] && c < ncol ? p.up_dlogits[(size_t)(row0 + rr) * n.N3 + 32 * nt + c] : 0.f;
                    }
                } else {
                    put_logit_tile(tile_dot<MT>(t.w3, (size_t)nt * KS2, h2, lane16), t.b3, nt, lt, r, h);
                    wave_fence();
                    if (lane < TILE) {
                        if (!walker) {
                            for (int c = 0; c < 32; c++) lt[r * LT + c] = 0.f;
                        } else {
                            for (int c = 0; c < ncol; c++) {
                                const float x = lt[r * LT + c];
                                if (a == 0) {
                                    hw = p.headws[(size_t)myrow * n.heads + hd];
                                    act = p.actions[source_row<IDX>(ri, r, myrow) * n.heads + hd];
                                }
                                float dl = 0.f;
                                if (n.multi || hd < p.num_active) {
                                    const float lpn = x - hw.x, pn = expf(lpn);
                                    const float lpo = p.old_logits[source_row<IDX>(ri, r, myrow) * n.N3 + 32 * nt + c] - hw.y, po = expf(lpo);
                                    kl_sum += po * (lpo - lpn);
                                    dl = c_lp * ((a == act ? 1.f : 0.f) - pn) + p.kl_coeff * (pn - po) + p.ent_coeff * (pn * (lpn + hw.z));
                                }
                                lt[r * LT + c] = dl;
                                if (++a == NA) { a = 0; hd++; }
                            }
                            for (int c = ncol; c < 32; c++) lt[r * LT + c] = 0.f;
                        }
                    }
                }
                wave_fence();
                // dlogits as bf16 [logit][rows] for dW3 (columns beyond N3 are zeros)
                for (int i = lane; i < TILE * 32; i += 64) {
                    const int c = i >> 5, rr = i & 31;
                    D3[(size_t)(32 * nt + c) * (size_t)ld + (size_t)(row0 + rr)] = (__bf16)lt[rr * LT + c];
                }
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    bf16x8 b;
#pragma unroll
                    for (int j = 0; j < 8; j++) b[j] = (__bf16)lt[r * LT + 16 * s + 8 * h + j];
                    uint4 q[MT];
#pragma unroll
                    for (int m = 0; m < MT; m++) q[m] = load_frag(w3b, ((size_t)m * NT3 + nt) * 2 + s, lane16);
#pragma unroll
                    for (int m = 0; m < MT; m++) dh[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(q[m]), b, dh[m], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                wave_fence();
            }
            if (!val) {
                s_kl = walker && !p.upstream ? kl_sum : 0.f;
                if (walker && p.o_kl && !p.upstream) p.o_kl[myrow] = kl_sum;
            }
        }

        // ---- dA2 = bf16(dH2 (.) act'(h2)), dH1^T = W2 dA2^T, dA1
        bf16x8 d2[MT][2];
        delta_frags<MT, RELU>(dh, h2, d2);
        store_frags<MT>(D2, ld, voff, d2);
        bf16x8 d1[MT][2];
#pragma unroll
        for (int m = 0; m < MT; m++) {
            const f32x16 g = tile_dot<MT>(w2b, (size_t)m * KS2, d2, lane16);
#pragma unroll
            for (int s = 0; s < 2; s++)
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const float hv = (float)h1[m][s][j], gv = g[8 * s + j];
                    d1[m][s][j] = (__bf16)(RELU ? (hv > 0.f ? gv : 0.f) : gv * (1.f - hv * hv));
                }
            asm volatile("" : "+v"(d1[m][0]), "+v"(d1[m][1]));
            __builtin_amdgcn_sched_barrier(0);
        }
        store_frags<MT>(D1, ld, voff, d1);
        }

        if (!p.fwd_only) {
            const double a0 = wave_sum(lane < TILE ? (double)s_surr : 0.), a1 = wave_sum(lane < TILE ? (double)s_kl : 0.);
            const double a2 = wave_sum(lane < TILE ? (double)s_ent : 0.), a3 = wave_sum(lane < TILE ? (double)s_vfl : 0.);
            if (lane == 0) {
                double *q = p.part + 4 * tile;
                q[0] = a0; q[1] = a1; q[2] = a2; q[3] = a3;
            }
        }
        wave_fence();
    }
