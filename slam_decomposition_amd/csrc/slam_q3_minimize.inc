// slam_q3_minimize.inc -- body of minimize_q3_kernel (slam_q3.hpp), minimize_ham_kernel (slam_ham_kernels.hpp) and minimize_hams_kernel (slam_hams.hpp): the quasi-Newton iteration of
// slam_long_minimize.inc (its body, copied) for one wavefront per item and n <= 2 * 64 parameters, n possibly odd.  Included inside the
// kernel with the constant STATE (and whatever its macros use) and three macros defined: Q3_MIN_SETUP declares n (and what the evaluation needs) from args
// and k, Q3_MIN_PROLOGUE fills the wavefront's LDS once per launch, Q3_MIN_EVAL is the evaluation -- x from lds[kQ3OffX ..], the loss
// returned, g into lds[kQ3OffG ..] -- with lds, tre, tim, k, n, wre, wim and args in scope.
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int k = args.k;
    Q3_MIN_SETUP
    float* f32a = reinterpret_cast<float*>(lds + kQ3OffF32);  // [NP] broadcast vector of the mat-vec: g'
    float* f32b = f32a + kQ3NP;                               // [NP] pending update: s
    float* f32c = f32b + kQ3NP;                               // [NP] pending update: v
    float2* const Hm = reinterpret_cast<float2*>(args.hmem + (size_t)blockIdx.x * (size_t)n * kQ3HStride) + lane;  // + j * 64: row j
    Q3_MIN_PROLOGUE
    const unsigned n_act = (unsigned)args.ctl->n_active;
    const unsigned n_items = n_act * (unsigned)args.restarts;
    const bool early = args.flags & 1u, ordered = args.flags & 2u;
    const int ent = ((lane & 7) * 8 + (lane >> 3)) * 2;
    unsigned rounds = 0;
    bool valid[kQ3Slots];
#pragma unroll
    for (int s = 0; s < kQ3Slots; ++s) valid[s] = 2 * lane + s < n;  // (n may be odd: slot n stays zero everywhere)
    const bool lane_in = 2 * lane < n;

    while (true) {
        unsigned pos = 0;
        if (lane == 0) pos = atomicAdd(&args.ctl->work_counter, 1u);
        pos = (unsigned)__builtin_amdgcn_readfirstlane((int)pos);
        if (pos >= n_items) break;
        const unsigned rs = pos / n_act;         // restart (restart-major queue: every target's restart r before any r + 1)
        const unsigned sl = pos - rs * n_act;    // target
        const unsigned item = sl * (unsigned)args.restarts + rs;
        const int mine = args.restarts - (int)rs;
        if (early) {
            const int fl = __hip_atomic_load(&args.solved[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ordered ? (fl > mine) : (fl != 0)) {  // a sibling restart has already succeeded (ordered: one with a lower index)
                if (lane == 0) item_rec_store_dropped(args.item_rec + item, ST_PREEMPTED);
#pragma unroll
                for (int s = 0; s < kQ3Slots; ++s)
                    if (valid[s]) args.item_x[(int64_t)item * n + 2 * lane + s] = 0.0;
                continue;
            }
        }
        const double2 tt = q3_item_entry<STATE>(args.targets, (int64_t)sl, lane, ent);
        const double tre = tt.x, tim = tt.y;
        double wre, wim;  // (the unitary is not wanted here)
        double x[kQ3Slots], g[kQ3Slots], p[kQ3Slots];
        {
            // start point: explicit, or Philox block `lane` = the parameter pair (2 lane, 2 lane + 1)
            double x0v[2] = {0.0, 0.0};
            if (lane_in) {
                if (args.x0) {
#pragma unroll
                    for (int s = 0; s < kQ3Slots; ++s)
                        if (valid[s]) x0v[s] = args.x0[(int64_t)item * n + 2 * lane + s];
                } else {
                    uint32_t w[4];
                    philox4x32_10((uint32_t)lane, rs, (uint32_t)((int)sl + (int)args.target_base), (uint32_t)k, (uint32_t)args.seed, (uint32_t)(args.seed >> 32), w);
                    x0v[0] = x0_from_words(w[0], w[1]);
                    x0v[1] = x0_from_words(w[2], w[3]);
                }
            }
#pragma unroll
            for (int s = 0; s < kQ3Slots; ++s) {
                x[s] = valid[s] ? x0v[s] : 0.0;
                lds[kQ3OffX + 2 * lane + s] = x[s];
            }
        }
        lds_fence();
        double f = Q3_MIN_EVAL;
        ++rounds;
        int nev = 1, nacc = 0, iters = 0, nback = 0, nstall = 0, status = ST_MAXITER;
        bool ident = true, scaled = false;  // ident: H is the identity (nothing of it is in memory yet)
        // The rank-2 update of an accepted step is applied by the NEXT step's mat-vec pass: pend = an update is waiting; its s and v in
        // LDS (f32b, f32c), this lane's components of w and s in registers
        bool pend = false;
        float pw0 = 0.0f, pw1 = 0.0f, ps0 = 0.0f, ps1 = 0.0f;
        double hs1 = 0.0, grow = 1.0;       // the effective metric is H + hs1 I (the one-off scaling of the initial metric)
        double gnorm = 0.0, gp = 0.0, pp = 0.0, alpha = 0.0;
        bool done = false;
        if (!isfinite(f)) {
            status = ST_NONFINITE;
            done = true;
        } else {
            nacc = 1;
            double gg = 0.0, gm = 0.0;
#pragma unroll
            for (int s = 0; s < kQ3Slots; ++s) {
                g[s] = valid[s] ? lds[kQ3OffG + 2 * lane + s] : 0.0;
                p[s] = -(double)(float)g[s];  // (the first direction is -H g with H = 1 in fp32)
                gm = max_abs(gm, g[s]);
            }
#pragma unroll
            for (int s = 0; s < kQ3Slots; ++s) gg = fma(g[s], p[s], gg);
            gp = wave_sum(gg);
            double d2 = 0.0;
#pragma unroll
            for (int s = 0; s < kQ3Slots; ++s) d2 = fma(p[s], p[s], d2);
            pp = wave_sum(d2);
            gnorm = wave_max_abs(gm);
            alpha = (pp > 1e-300) ? fmin(grow, kStepMax * fast_rsqrt(pp)) : grow;
            if (f < args.stop_loss || gnorm < args.gtol || (gnorm < args.gtol_far && f > args.far_loss)) { status = ST_CONVERGED; done = true; }
            else if (args.maxiter <= 0) { status = ST_MAXITER; done = true; }
        }
        while (!done) {
            // ---- trial point
            double xt[kQ3Slots];
#pragma unroll
            for (int s = 0; s < kQ3Slots; ++s) {
                xt[s] = fma(alpha, p[s], x[s]);
                lds[kQ3OffX + 2 * lane + s] = xt[s];
            }
            lds_fence();
            const double ft = Q3_MIN_EVAL;
            ++rounds;
            ++nev;
            const bool finite = isfinite(ft);
            const bool armijo = finite && (ft <= f + kArmijoC1 * alpha * gp);
            if (armijo) {
                ++nacc;
                double gt[kQ3Slots], qv[kQ3Slots];
                double pgt = 0.0, yy = 0.0, gm = 0.0;
#pragma unroll
                for (int s = 0; s < kQ3Slots; ++s) {
                    gt[s] = valid[s] ? lds[kQ3OffG + 2 * lane + s] : 0.0;
                    const double ya = gt[s] - g[s];
                    pgt = fma(p[s], gt[s], pgt);
                    yy = fma(ya, ya, yy);
                    gm = max_abs(gm, gt[s]);
                }
                pgt = wave_sum(pgt);
                yy = wave_sum(yy);
                // ---- q = H g' (fp32), H = the matrix in memory (or the identity) + the pending update: one pass over the rows
                if (ident && !pend) {
#pragma unroll
                    for (int s = 0; s < kQ3Slots; ++s) qv[s] = (double)(float)gt[s];
                } else {
                    f32a[2 * lane] = (float)gt[0];
                    f32a[2 * lane + 1] = (float)gt[1];
                    lds_fence();
                    float a0 = 0.0f, a1 = 0.0f, b0 = 0.0f, b1 = 0.0f;  // two accumulator pairs: even / odd rows
                    if (lane_in) {
                        for (int j0 = 0; j0 < n; j0 += kQ3RowBatch) {
                            float2 h[kQ3RowBatch];
#pragma unroll
                            for (int u = 0; u < kQ3RowBatch; ++u) {
                                const int j = j0 + u;
                                if (ident) h[u] = make_float2(j == 2 * lane ? 1.0f : 0.0f, (j == 2 * lane + 1 && valid[1]) ? 1.0f : 0.0f);
                                else if (j < n) h[u] = Hm[(size_t)j * 64];
                                else h[u] = make_float2(0.0f, 0.0f);
                            }
                            if (pend) {
#pragma unroll
                                for (int u = 0; u < kQ3RowBatch; ++u) {
                                    const int j = j0 + u;
                                    const float sj = f32b[j], vj = f32c[j];
                                    h[u].x = fmaf(vj, ps0, h[u].x); h[u].y = fmaf(vj, ps1, h[u].y);
                                    h[u].x = fmaf(sj, pw0, h[u].x); h[u].y = fmaf(sj, pw1, h[u].y);
                                    if (j < n) Hm[(size_t)j * 64] = h[u];
                                }
                            }
#pragma unroll
                            for (int u = 0; u < kQ3RowBatch; u += 2) {
                                const float g0 = f32a[j0 + u], g1 = f32a[j0 + u + 1];  // (rows beyond n: g' = 0 there; the vectors have kQ3NP entries)
                                a0 = fmaf(h[u].x, g0, a0); a1 = fmaf(h[u].y, g0, a1);
                                b0 = fmaf(h[u + 1].x, g1, b0); b1 = fmaf(h[u + 1].y, g1, b1);
                            }
                        }
                    }
                    if (pend) ident = false;  // the matrix is in memory now
                    pend = false;
                    qv[0] = (double)(a0 + b0);
                    qv[1] = (double)(a1 + b1);
                    lds_fence();
                }
                const double sg = alpha * pgt;
                const double sy = alpha * (pgt - gp);
                const double ss = (alpha * alpha) * pp;
                const bool too_short = sy < (1.0 - kWolfeC2) * alpha * (-gp);  // weak-Wolfe curvature condition violated
                const bool curv = !too_short && sy > 0.0 && (sy * sy > (kCurvEps * kCurvEps) * (ss * yy));
                const bool first = curv && !scaled;
                scaled = scaled || curv;
                // first update of an item: scale the initial metric (the identity) by s.y / y.y -- as the scalar hs1
                const double fac = first ? (sy * fast_rcp(yy)) : 1.0;
                hs1 = first ? fac - 1.0 : hs1;
                double yu = 0.0;
#pragma unroll
                for (int s = 0; s < kQ3Slots; ++s) {
                    qv[s] = fma(hs1, gt[s], qv[s]);  // q = H_eff g'
                    const double ua = fma(fac, p[s], qv[s]);  // u = H_eff y = q + fac p   (p = -H_eff g before this round's scaling)
                    yu = fma(gt[s] - g[s], ua, yu);
                }
                yu = wave_sum(yu);
                const double rho = curv ? fast_rcp(sy) : 0.0;
                const double cf = rho * (1.0 + rho * yu);
                double wg = 0.0;
                double sa[kQ3Slots], wa[kQ3Slots], va[kQ3Slots];
#pragma unroll
                for (int s = 0; s < kQ3Slots; ++s) {
                    sa[s] = alpha * p[s];
                    const double ua = fma(fac, p[s], qv[s]);
                    wa[s] = cf * sa[s] - rho * ua;
                    va[s] = -rho * ua;
                    wg = fma(wa[s], gt[s], wg);
                }
                wg = wave_sum(wg);
                // ---- H += s w^T + v s^T (fp32; row j gets s_j w + v_j s): left pending for the next accepted step's pass
                if (curv) {
                    f32b[2 * lane] = (float)sa[0];
                    f32b[2 * lane + 1] = (float)sa[1];
                    f32c[2 * lane] = (float)va[0];
                    f32c[2 * lane + 1] = (float)va[1];
                    pw0 = (float)wa[0]; pw1 = (float)wa[1];
                    ps0 = (float)sa[0]; ps1 = (float)sa[1];
                    pend = true;
                    lds_fence();
                }
                nstall = (f - ft <= kStallDf) ? nstall + 1 : 0;
                f = ft;
                ++iters;
                nback = 0;
                grow = too_short ? fmin(grow * kGrowFactor, kGrowMax) : 1.0;
                double d1 = 0.0, d2 = 0.0;
#pragma unroll
                for (int s = 0; s < kQ3Slots; ++s) {
                    x[s] = xt[s];
                    g[s] = gt[s];
                    p[s] = -(qv[s] + sa[s] * wg + va[s] * sg);
                    d1 = fma(g[s], p[s], d1);
                    d2 = fma(p[s], p[s], d2);
                }
                gnorm = wave_max_abs(gm);
                gp = wave_sum(d1);
                pp = wave_sum(d2);
                alpha = (pp > 1e-300) ? fmin(grow, kStepMax * fast_rsqrt(pp)) : grow;
                if (f < args.stop_loss || gnorm < args.gtol || (gnorm < args.gtol_far && f > args.far_loss)) { status = ST_CONVERGED; done = true; }
                else if (nstall >= 2) { status = ST_STALLED; done = true; }
                else if (iters >= args.maxiter) { status = ST_MAXITER; done = true; }
                // not a descent direction (H lost positive definiteness numerically), or the periodic restart: steepest descent again
                const bool periodic = !done && ((iters & (kRestartPeriod - 1)) == 0);
                if (!done && (!(gp < 0.0) || periodic)) {
                    ident = true;
                    pend = false;
                    hs1 = 0.0;
                    scaled = periodic ? false : scaled;
                    double gg = 0.0;
#pragma unroll
                    for (int s = 0; s < kQ3Slots; ++s) {
                        p[s] = -g[s];
                        gg = fma(g[s], g[s], gg);
                    }
                    gg = wave_sum(gg);
                    gp = -gg;
                    pp = gg;
                    alpha = periodic ? ((gg > 1e-300) ? fmin(grow, kStepMax * fast_rsqrt(gg)) : grow) : alpha;
                }
            } else {
                // safeguarded quadratic interpolation backtrack
                const double denom = 2.0 * (ft - f - gp * alpha);
                const double anew = (finite && denom > 0.0 && isfinite(denom)) ? (-gp * alpha * alpha * fast_rcp(denom)) : 0.5 * alpha;
                alpha = fmin(fmax(anew, 0.1 * alpha), 0.5 * alpha);
                grow = 1.0;
                ++nback;
                if (nback > kMaxBacktrack) { status = (gnorm < kStallGnorm) ? ST_STALLED : ST_LINESEARCH; done = true; }
            }
            // ---- early exit across the restarts of one target (optimizer.py:287-295)
            if (early && !done) {
                const int fl = __hip_atomic_load(&args.solved[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (ordered ? (fl > mine) : (fl != 0)) { status = ST_PREEMPTED; done = true; }
            }
        }
        if (early && status != ST_PREEMPTED && f < args.exit_loss && lane == 0)
            __hip_atomic_fetch_max(&args.solved[sl], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0) item_rec_store(args.item_rec + item, f, iters, status, nev, nacc);
#pragma unroll
        for (int s = 0; s < kQ3Slots; ++s)
            if (valid[s]) args.item_x[(int64_t)item * n + 2 * lane + s] = x[s];
    }
    if (lane == 0 && rounds) atomicAdd(&args.ctl->rounds, (unsigned long long)rounds);
