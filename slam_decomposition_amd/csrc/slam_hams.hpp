// slam_hams.hpp -- time-sliced Hamiltonian templates: fit the parameters x of a piecewise-constant pulse (gfx950 only),
//
//   U(x) = U_S ... U_2 U_1,   U_s = exp(-i (t / S) H_s(x)),   H_s(x) = sum_k c_{s,k} M_k + h.c.,
//   c_{s,k} = x[s_index[s][k]] exp(i x[phi_index[s][k]])  (phi_index = -1: phase 0),   t = x[t_index]  (t_index = -1: t = 1),
//
// slice 1 acting first, S <= 8.  ONE WAVEFRONT per (target, restart) item, lane l holds entry (r = l & 7, c = l >> 3) of every 8x8, dim = 4
// as the leading block of the 8x8: everything as in slam_ham.hpp, whose Jacobi step, sinc series, 8-term products, entry-list evaluation
// and cost map are used here.  A parameter may feed any number of slices; its derivative is the sum over the slices that read it.
//
// Evaluation (eval_hams), with P_s = U_s ... U_1 (P_0 = 1), Q_s = U_S ... U_s (Q_{S+1} = 1), z = Tr(T^+ U) / d:
//   forward, s = 1 .. S:   H_s from the slice's entry lists, H_s = V_s diag(lambda_s) V_s^+ (Jacobi), U_s = V_s e_s V_s^+, P_s = U_s P_{s-1};
//                          V_s, lambda_s and e_s go to the wavefront's workspace in device memory (all but the last slice's, which stay in LDS);
//   then U = P_S, z, the loss and sigma (d loss = Re(sigma dz));
//   backward, s = S .. 1:  with R = T^+ Q_{s+1} (R = T^+ at s = S) and P = P_s: V_s, lambda_s and e_s come back from the workspace,
//                          P_{s-1} = U_s^+ P,  T_s^+ = P_{s-1} R,  B = V_s^+ T_s^+ V_s,  Phi with tau = t / S in the place of t,
//                          K = V_s (B o Phi) V_s^+ and the single-exponential gradient formula; R <- R U_s.
//                          dz/dt = (1 / S) sum_s (1 / d) sum_a B^s_aa (-i lambda^s_a) e^s_a.
// The backward sweep makes no second eigen-solve and keeps no per-slice state in LDS: five 1 KB matrices (V, two temporaries, P, R) take
// the place of the q3 kernels' trig and gate tables, the entry lists (per slice) are read from device memory, and a wavefront's LDS stays
// kQ3LdsBytes.  The optimizer is slam_q3_minimize.inc around eval_hams; start points always come from the host (x0).
//
// Reference behaviour: ConversionGainSmush / ConversionGainSmush1QPhase src/slam/hamiltonian.py:114-182 (totalUi = Ui @ totalUi).
#pragma once
#include "slam_ham.hpp"

namespace slamdev {

constexpr int kHamsMaxSlices = 8;
constexpr int kHamsWorkSlice = 128 + 8 + 16;                  // doubles of one slice in the workspace: V [64] double2, lambda [8], e [8] double2
constexpr int kHamsWorkDoubles = (kHamsMaxSlices - 1) * kHamsWorkSlice;  // per wavefront (the last slice is never stored)

// LDS: the layout of slam_ham.hpp without its entry lists; P and R in their place
constexpr int kHamsOffP = kHamOffM2 + 128;  // the running prefix product P_s
constexpr int kHamsOffR = kHamsOffP + 128;  // the running T^+ Q_{s+1}
static_assert(kHamsOffR + 128 <= kQ3OffF32, "the five matrices fit between the gradient and the metric pass's vectors");

struct HamsDesc {
    const double* w;        // [S][64][2][2]
    const uint32_t* idx;    // [S][64], packed as in HamDesc
    double* work;           // [wavefronts][kHamsWorkDoubles]
    uint32_t reads[kHamsMaxSlices];  // bit j: slice s reads parameter j
    int32_t n, t_index, dim, n_slices;
};
struct HamsArgs : Q3Args {  // (gates, edges: unused; k = 0)
    HamsDesc h;
};
struct HamsEvalArgs {
    const double* targets;    // [n_targets][8][8][2], zero-padded for dim = 4
    const double* x;          // [M][n]
    const int32_t* target_of; // [M]
    int64_t n_items;
    double* loss;
    double* grad;             // [M][n] or nullptr
    double* unitary;          // [M][8][8][2] or nullptr
    int32_t cost_kind;
    HamsDesc h;
};

__device__ __forceinline__ void hams_prologue(double* lds) {
    load_sincos_table(reinterpret_cast<double2*>(lds + kQ3OffTbl), threadIdx.x);
    lds_fence();
}

// the sweeps of eval_ham over ham_jacobi_step: in the lane's entry of H; out its entry of V, and lambda_r on the diagonal lanes' ar
__device__ __forceinline__ void hams_jacobi(double* lds, int r, int c, double& ar, double& ai, double& vr, double& vi) {
    vr = (r == c) ? 1.0 : 0.0;
    vi = 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kHamMaxSweeps; ++sweep) {
        const double a2 = fma(ar, ar, ai * ai);
        const double off2 = wave_sum(r == c ? 0.0 : a2), all2 = wave_sum(a2);
        if (!(off2 > 1e-30 * all2)) break;
        ham_jacobi_step<1>(lds, r, c, ar, ai, vr, vi);
        ham_jacobi_step<2>(lds, r, c, ar, ai, vr, vi);
        ham_jacobi_step<3>(lds, r, c, ar, ai, vr, vi);
        ham_jacobi_step<4>(lds, r, c, ar, ai, vr, vi);
        ham_jacobi_step<5>(lds, r, c, ar, ai, vr, vi);
        ham_jacobi_step<6>(lds, r, c, ar, ai, vr, vi);
        ham_jacobi_step<7>(lds, r, c, ar, ai, vr, vi);
        if (off2 <= 1e-22 * all2) break;
    }
}

// Between two products that do not depend on each other: the scheduler would otherwise issue the LDS reads of both (32 registers each) ahead
// of the arithmetic of the first
__device__ __forceinline__ void hams_one_at_a_time() { __builtin_amdgcn_sched_barrier(0); }

// the lane's entry of V diag(e) V^+
__device__ __forceinline__ void hams_vev(const double2* v, const double2* ev, int r, int c, double& outr, double& outi) {
    double accr = 0.0, acci = 0.0;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const double2 x = v[r * 8 + a], y = v[c * 8 + a], e = ev[a];
        const double pr = fma(x.x, e.x, -(x.y * e.y)), pim = fma(x.x, e.y, x.y * e.x);
        accr = fma(pr, y.x, fma(pim, y.y, accr));
        acci = fma(pim, y.x, fma(-pr, y.y, acci));
    }
    outr = accr;
    outi = acci;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Fused loss + gradient of one item by the whole wavefront.  In: the trial point in lds[kQ3OffX ..], this lane's target entry
// T[r][c] (zero outside the leading dim x dim block).  Out: the loss (wave-uniform), the gradient in lds[kQ3OffG ..], this lane's
// entry of U in (wre, wim).
// ---------------------------------------------------------------------------------------------------------------------------
template <bool HUGE_ARGS>
__device__ __forceinline__ double eval_hams(double* lds, double tre, double tim, const HamsDesc& h, int cost_kind, double& wre, double& wim) {
    const int lane = threadIdx.x;
    const int r = lane & 7, c = lane >> 3;
    const bool diag = r == c;
    const int S = h.n_slices, n = h.n, t_index = h.t_index;
    const double2* tbl = reinterpret_cast<const double2*>(lds + kQ3OffTbl);
    const double* xs = lds + kQ3OffX;
    double* gs = lds + kQ3OffG;
    double* lam = lds + kHamOffLam;
    double2* ev = reinterpret_cast<double2*>(lds + kHamOffE);
    double2* m0 = reinterpret_cast<double2*>(lds + kHamOffM0);
    double2* m1 = reinterpret_cast<double2*>(lds + kHamOffM1);
    double2* m2 = reinterpret_cast<double2*>(lds + kHamOffM2);
    double2* mp = reinterpret_cast<double2*>(lds + kHamsOffP);
    double2* mr = reinterpret_cast<double2*>(lds + kHamsOffR);
    double* work = h.work + (size_t)blockIdx.x * kHamsWorkDoubles;
    const double2* w2 = reinterpret_cast<const double2*>(h.w) + 2 * lane;
    auto sc = [&](double arg, double& s, double& co) {
        if constexpr (HUGE_ARGS) sincos_any(arg, tbl, s, co);
        else sincos_tbl(arg, tbl, s, co);
    };
    const double t = t_index >= 0 ? xs[t_index >= 0 ? t_index : 0] : 1.0;
    const double inv_s = 1.0 / (double)S;
    const double tau = t / (double)S;
    const double inv_d = h.dim == 4 ? 0.25 : 0.125;
    // ---- forward: P_s = U_s P_{s-1}
    double pre = 0.0, pim = 0.0;  // the lane's entry of P_s
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
        HamEntry en;
        double ar, ai, vr, vi;
        ham_entry<HUGE_ARGS>(h.idx[s * 64 + lane], w2 + s * 128, xs, tbl, en, ar, ai);
        hams_jacobi(lds, r, c, ar, ai, vr, vi);
        if (diag) lam[r] = ar;
        m0[r * 8 + c] = make_double2(vr, vi);
        double sn, cs;
        sc(tau * ar, sn, cs);
        if (diag) ev[r] = make_double2(cs, -sn);
        lds_fence();
        if (s < S - 1) {
            reinterpret_cast<double2*>(work + s * kHamsWorkSlice)[lane] = make_double2(vr, vi);
            if (lane < 8) {
                work[s * kHamsWorkSlice + 128 + lane] = lam[lane];
                reinterpret_cast<double2*>(work + s * kHamsWorkSlice + 136)[lane] = ev[lane];
            }
        }
        double ur, ui;
        hams_vev(m0, ev, r, c, ur, ui);
        if (s > 0) {
            m1[r * 8 + c] = make_double2(ur, ui);
            lds_fence();
            ham_dot8<false, false>(m1 + r * 8, 1, mp + c, 8, pre, pim);
            lds_fence();
        } else {
            pre = ur;
            pim = ui;
        }
        mp[r * 8 + c] = make_double2(pre, pim);
        lds_fence();
    }
    wre = pre;
    wim = pim;
    // ---- z = (1/d) sum conj(T[r][c]) U[r][c], the loss, sigma
    const double zr = wave_sum(fma(tre, pre, tim * pim)) * inv_d, zi = wave_sum(fma(tre, pim, -(tim * pre))) * inv_d;
    double sr, sim;
    const double fout = ham_cost(zr, zi, h.dim, cost_kind, sr, sim);
    // ---- backward: R = T^+ Q_{s+1}, P = P_s; V, lambda and e of the last slice are still in LDS
    mr[c * 8 + r] = make_double2(tre, -tim);
    lds_fence();
    double mine = 0.0, gt = 0.0;
#pragma unroll 1
    for (int s = S - 1; s >= 0; --s) {
        if (s < S - 1) {
            const double* ws = work + s * kHamsWorkSlice;
            m0[r * 8 + c] = reinterpret_cast<const double2*>(ws)[lane];
            if (lane < 8) {
                lam[lane] = ws[128 + lane];
                ev[lane] = reinterpret_cast<const double2*>(ws + 136)[lane];
            }
            lds_fence();
        }
        // B = V^+ P_{s-1} R V; on the way P <- P_{s-1} = U_s^+ P and, once R V is taken, R <- R U_s
        double xr, xi, br, bi;
        ham_dot8<false, false>(mr + r * 8, 1, m0 + c, 8, xr, xi);
        if (s > 0) {
            double ur, ui, npr, npi, nrr, nri;
            hams_one_at_a_time();
            hams_vev(m0, ev, r, c, ur, ui);
            m1[r * 8 + c] = make_double2(ur, ui);
            lds_fence();
            ham_dot8<true, false>(m1 + r, 8, mp + c, 8, npr, npi);       // P_{s-1}[r][c] = sum_k conj(U[k][r]) P[k][c]
            hams_one_at_a_time();
            ham_dot8<false, false>(mr + r * 8, 1, m1 + c, 8, nrr, nri);  // (R U)[r][c]
            lds_fence();
            mp[r * 8 + c] = make_double2(npr, npi);
            mr[r * 8 + c] = make_double2(nrr, nri);
            m2[r * 8 + c] = make_double2(xr, xi);
            lds_fence();
            ham_dot8<false, false>(mp + r * 8, 1, m2 + c, 8, xr, xi);
        }  // (P_0 = 1)
        m1[r * 8 + c] = make_double2(xr, xi);
        lds_fence();
        ham_dot8<true, false>(m0 + r, 8, m1 + c, 8, br, bi);
        const double lr = lam[r], lc = lam[c];
        const double hs = 0.5 * tau * (lr + lc), hd = 0.5 * tau * (lr - lc);
        double sn_s, cs_s, sn_d, cs_d;
        sc(hs, sn_s, cs_s);
        sc(hd, sn_d, cs_d);
        const double snc = ham_sinc(hd, sn_d);
        const double fr = cs_s * snc, fi = -sn_s * snc;                        // Phi[r][c]
        const double qr = fma(br, fr, -(bi * fi)), qi = fma(br, fi, bi * fr);  // (B o Phi)[r][c]
        const double dtr = wave_sum(diag ? lr * qr : 0.0) * inv_d, dti = wave_sum(diag ? lr * qi : 0.0) * inv_d;
        gt += fma(sr, dti, sim * dtr);  // Re(sigma (-i)(dtr + i dti))
        // K = V (B o Phi) V^+, this lane's K[c][r]
        lds_fence();
        m1[r * 8 + c] = make_double2(qr, qi);
        lds_fence();
        double yr, yi, kr, ki;
        ham_dot8<false, true>(m1 + r * 8, 1, m0 + c * 8, 1, yr, yi);
        m2[r * 8 + c] = make_double2(yr, yi);
        lds_fence();
        ham_dot8<false, false>(m0 + c * 8, 1, m2 + r, 8, kr, ki);
        // kappa = sigma (-i tau / d) K[c][r]
        const double fr_ = tau * inv_d * sim, fi_ = -(tau * inv_d * sr);
        const double kar = fma(fr_, kr, -(fi_ * ki)), kai = fma(fr_, ki, fi_ * kr);
        HamEntry en;
        double ar, ai, gstr[2], gphi[2];
        ham_entry<HUGE_ARGS>(h.idx[s * 64 + lane], w2 + s * 128, xs, tbl, en, ar, ai);
        ham_entry_grad(en, kar, kai, gstr, gphi);
        uint32_t bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.reads[s]);
#pragma unroll 1
        while (bits) {
            const int j = __builtin_ctz(bits);
            bits &= bits - 1u;
            double v;
            ham_entry_share(en, gstr, gphi, j, v);
            const double tot = wave_sum(v);
            if (lane == j) mine += tot;
        }
        lds_fence();
    }
    if (lane == t_index) mine = fma(gt, inv_s, mine);
    if (lane < n) gs[lane] = mine;
    lds_fence();
    return fout;
}

// ---------------------------------------------------------------------------------------------------------------------------
// slam_hams_eval: one item per wavefront, grid-stride
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWave, 2) eval_hams_kernel(HamsEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int n = a.h.n;
    hams_prologue(lds);
    const int ent = ((lane & 7) * 8 + (lane >> 3)) * 2;  // entry (r, c) of a row-major 8x8
    for (int64_t m = blockIdx.x; m < a.n_items; m += gridDim.x) {
#pragma unroll
        for (int s = 0; s < kQ3Slots; ++s) {
            const int i = 2 * lane + s;
            lds[kQ3OffX + i] = i < n ? a.x[m * n + i] : 0.0;
        }
        lds_fence();
        const double2 t = q3_item_entry<false>(a.targets, (int64_t)a.target_of[m], lane, ent);
        double wr = 0.0, wi = 0.0;
        const double f = eval_hams<true>(lds, t.x, t.y, a.h, a.cost_kind, wr, wi);
        if (lane == 0) a.loss[m] = f;
        if (a.grad && lane < n) a.grad[m * n + lane] = lds[kQ3OffG + lane];
        if (a.unitary) *reinterpret_cast<double2*>(a.unitary + m * 128 + ent) = make_double2(wr, wi);
        lds_fence();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// slam_hams_minimize: the optimizer body of the three-qubit templates around eval_hams
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWave, 3) minimize_hams_kernel(HamsArgs args) {
    constexpr bool STATE = false;
#define Q3_MIN_SETUP const int n = args.h.n;
#define Q3_MIN_PROLOGUE hams_prologue(lds);
#define Q3_MIN_EVAL eval_hams<false>(lds, tre, tim, args.h, args.cost_kind, wre, wim)
#include "slam_q3_minimize.inc"
#undef Q3_MIN_SETUP
#undef Q3_MIN_PROLOGUE
#undef Q3_MIN_EVAL
}

}  // namespace slamdev
