// slam_ham.hpp -- Hamiltonian templates: fit the drive parameters x of U(x) = exp(-i t H(x)) to a target (gfx950 only).  ONE WAVEFRONT
// per (target, restart) item, lane l holds entry (r = l & 7, c = l >> 3) of every 8x8, as in slam_q3.hpp.
//
//   H(x) = sum_k c_k M_k + h.c.,  c_k = x[s_k] exp(i x[phi_k])  (phi_k = -1: phase 0),  t = x[t_index]  (t_index = -1: t = 1),
// M_k dense dim x dim, dim = 4 or 8, n <= 32 parameters, <= 16 terms.  dim = 4 runs as the leading 4x4 block of an 8x8 whose other
// entries are zero: U = diag(U4, I), the zero-padded target contributes nothing, and the loss divides by d = 4.
//
// Evaluation (eval_ham):
//   1. the lane's entry of H from x: the host has compressed the M_k into per-entry lists of at most two contributions
//      (strength index, phase index, conjugate flag, complex weight), kept in LDS;
//   2. H = V diag(lambda) V^+ by a parallel Jacobi iteration: for m = 1 .. 7 the pairs (i, i ^ m) are four disjoint rotations and the
//      seven masks cover all 28 pairs, so a sweep is seven steps; a step's partners are lane XORs (m on the row, m << 3 on the column
//      index).  The sweep loop is wave-uniform, stops on the off-diagonal norm and is capped at kHamMaxSweeps;
//   3. with B = V^+ T^+ V and e_a = exp(-i t lambda_a):  z = (1/d) sum_a B_aa e_a;  BasicCost = 1 - |z|, SquareCost its scalar map;
//   4. gradient: Phi_ab = exp(-i t (l_a + l_b) / 2) sinc(t (l_a - l_b) / 2) (sin(u) / u as a series in u^2 near 0: nothing divides by an
//      eigenvalue gap), K = V (B o Phi) V^+, dz/dx_j = (-i t / d) Tr(K dH/dx_j), dz/dt = (1/d) sum_a B_aa (-i l_a) e_a; for a term
//      dH/ds = e^{i phi} M + h.c., dH/dphi = i s e^{i phi} M + h.c.; contributions to one parameter index add.  The formula holds for
//      any eigenbasis of a degenerate eigenvalue.
// The 8x8 products go through three LDS matrices of 1 KB in the areas the q3 kernels use for their trig and gate tables; the LDS of a
// wavefront stays kQ3LdsBytes.  The optimizer is slam_q3_minimize.inc around eval_ham; start points always come from the host (x0).
// This header holds __device__ functions only (slam_hams.hpp uses them too); the two kernels are in slam_ham_kernels.hpp.
//
// Reference behaviour: HamiltonianTemplate src/slam/basis.py:24-48, src/slam/hamiltonian.py; BasicCost / SquareCost
// src/slam/cost_function.py:140-145,169-173.
#pragma once
#include "slam_q3.hpp"

namespace slamdev {

constexpr int kHamMaxTerms = 16;
constexpr int kHamMaxParams = 32;
constexpr int kHamMaxSweeps = 12;

// LDS of one wavefront, in doubles, inside the q3 layout: x[128] and g[128] keep their places (n <= 32: the 96 doubles behind g[32]
// are free), the three fp32 vectors of the metric pass too; the trig and gate-table areas hold the matrices and the entry lists
constexpr int kHamOffLam = kQ3OffG + kHamMaxParams;  // [8] the diagonal of the running matrix / the eigenvalues
constexpr int kHamOffRot = kHamOffLam + 8;           // [8][4] per index i of a step: cos, Re o_i, Im o_i, -- (o_i = J[i ^ m][i])
constexpr int kHamOffE = kHamOffRot + 32;            // [8] double2 e_a
static_assert(kHamOffE + 16 <= kQ3OffG + kQ3NP, "the small areas fit behind g[32]");
constexpr int kHamOffM0 = kQ3OffTrig;                // V
constexpr int kHamOffM1 = kHamOffM0 + 128;           // T, then B o Phi
constexpr int kHamOffM2 = kHamOffM1 + 128;           // T^+ V, then (B o Phi) V^+
constexpr int kHamOffW = kHamOffM2 + 128;            // [64][2] double2: the weights of the lane's two contributions
constexpr int kHamOffIdx = kHamOffW + 256;           // [64] uint32: their packed indices
static_assert(kHamOffIdx + 32 <= kQ3OffF32, "matrices and entry lists fit between the gradient and the metric pass's vectors");
static_assert(kHamOffM0 % 2 == 0 && kHamOffRot % 2 == 0 && kHamOffE % 2 == 0, "double2 alignment");

// packed indices of a lane's two contributions q = 0, 1 (bits 16 q ..): bits 0-5 strength index + 1 (0: no contribution), bits 6-11
// phase index + 1 (0: phase 0), bit 12: the conjugate half (e^{-i phi} conj(M[c][r]))
struct HamDesc {
    const double* w;        // [64][2][2]
    const uint32_t* idx;    // [64]
    int32_t n, t_index, dim;
};
struct HamArgs : Q3Args {   // (gates, edges: unused; k = 0)
    HamDesc h;
};
struct HamEvalArgs {
    const double* targets;    // [n_targets][8][8][2], zero-padded for dim = 4
    const double* x;          // [M][n]
    const int32_t* target_of; // [M]
    int64_t n_items;
    double* loss;
    double* grad;             // [M][n] or nullptr
    double* unitary;          // [M][8][8][2] or nullptr
    int32_t cost_kind;
    HamDesc h;
};

// the value of lane (l ^ MASK): within 32 lanes one ds_swizzle (bit mode), across the halves ds_bpermute
template <int MASK>
__device__ __forceinline__ double ham_xor(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    if constexpr (MASK < 32) {
        lo = __builtin_amdgcn_ds_swizzle(lo, 0x1F | (MASK << 10));
        hi = __builtin_amdgcn_ds_swizzle(hi, 0x1F | (MASK << 10));
    } else {
        const int addr = ((int)threadIdx.x ^ MASK) << 2;
        lo = __builtin_amdgcn_ds_bpermute(addr, lo);
        hi = __builtin_amdgcn_ds_bpermute(addr, hi);
    }
    return __hiloint2double(hi, lo);
}

// sum_k A_k B_k, A_k = a[k as] (conjugated: CA), B_k = b[k bs] (conjugated: CB)
template <bool CA, bool CB>
__device__ __forceinline__ void ham_dot8(const double2* a, int as, const double2* b, int bs, double& outr, double& outi) {
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double2 x = a[k * as], y = b[k * bs];
        const double xi = CA ? -x.y : x.y, yi = CB ? -y.y : y.y;
        sr = fma(x.x, y.x, fma(-xi, yi, sr));
        si = fma(x.x, yi, fma(xi, y.x, si));
    }
    outr = sr;
    outi = si;
}

// One Jacobi step: the four rotations of the pairs (i, i ^ M) at once, A <- J^+ A J, V <- V J.  For the pair p < q with b = A[p][q],
// e = b / |b|, tau = (A[q][q] - A[p][p]) / (2 |b|), t = sign(tau) / (|tau| + sqrt(1 + tau^2)), c = 1 / sqrt(1 + t^2), s = t c:
// J[p][p] = J[q][q] = c, J[p][q] = s e, J[q][p] = -s conj(e).  The lane (p, q) computes them and stores, per index i, c and
// o_i = J[i ^ M][i]; |b|^2 <= 1e-300 (b = 0: the padding of dim = 4, H = 0, a converged pair): no rotation.
template <int M>
__device__ __forceinline__ void ham_jacobi_step(double* lds, int r, int c, double& ar, double& ai, double& vr, double& vi) {
    double* lam = lds + kHamOffLam;
    double* rot = lds + kHamOffRot;
    if (r == c) lam[r] = ar;
    lds_fence();
    {
        const int q = r ^ M;
        const double a = lam[r], d = lam[q];
        const double b2 = fma(ar, ar, ai * ai);
        const bool turn = b2 > 1e-300;
        const double ib = turn ? fast_rsqrt(b2) : 0.0;
        const double tau = (d - a) * 0.5 * ib;
        const double t = copysign(1.0 / (fabs(tau) + sqrt(fma(tau, tau, 1.0))), tau);  // (tau = +-inf: t = 0)
        const double cs = turn ? fast_rsqrt(fma(t, t, 1.0)) : 1.0;
        const double sn = turn ? t * cs : 0.0;
        const double er = ar * ib, ei = ai * ib;
        if (c == q && r < q) {
            rot[4 * r] = cs;
            rot[4 * r + 1] = -sn * er;
            rot[4 * r + 2] = sn * ei;
            rot[4 * q] = cs;
            rot[4 * q + 1] = sn * er;
            rot[4 * q + 2] = sn * ei;
        }
    }
    lds_fence();
    const double cc = rot[4 * c], ocr = rot[4 * c + 1], oci = rot[4 * c + 2];
    const double cr = rot[4 * r], orr = rot[4 * r + 1], ori = rot[4 * r + 2];
    // X = A J, V <- V J: the lane's entry and the one of column c ^ M
    const double pcr = ham_xor<(M << 3)>(ar), pci = ham_xor<(M << 3)>(ai);
    const double pvr = ham_xor<(M << 3)>(vr), pvi = ham_xor<(M << 3)>(vi);
    const double xr = fma(ar, cc, fma(pcr, ocr, -(pci * oci)));
    const double xi = fma(ai, cc, fma(pcr, oci, pci * ocr));
    const double nvr = fma(vr, cc, fma(pvr, ocr, -(pvi * oci)));
    const double nvi = fma(vi, cc, fma(pvr, oci, pvi * ocr));
    vr = nvr;
    vi = nvi;
    // A <- J^+ X: the lane's entry and the one of row r ^ M, with conj(o_r)
    const double pxr = ham_xor<M>(xr), pxi = ham_xor<M>(xi);
    ar = fma(cr, xr, fma(orr, pxr, ori * pxi));
    ai = fma(cr, xi, fma(orr, pxi, -(ori * pxr)));
}

// sin(u) / u: below |u| = 1/2 the series sum_k (-1)^k u^(2k) / (2k + 1)!, nine terms (the first one left out is below 2e-22)
__device__ __forceinline__ double ham_sinc(double u, double sin_u) {
    const double u2 = u * u;
    double p = 1.0 / 355687428096000.0;  // 1 / 17!
    p = fma(p, u2, -1.0 / 1307674368000.0);
    p = fma(p, u2, 1.0 / 6227020800.0);
    p = fma(p, u2, -1.0 / 39916800.0);
    p = fma(p, u2, 1.0 / 362880.0);
    p = fma(p, u2, -1.0 / 5040.0);
    p = fma(p, u2, 1.0 / 120.0);
    p = fma(p, u2, -1.0 / 6.0);
    p = fma(p, u2, 1.0);
    const bool small = u2 < 0.25;
    return small ? p : sin_u / (small ? 1.0 : u);
}

// BasicCost / SquareCost of z = Tr(T^+ U) / d, and sigma = sr + i sim with d loss = Re(sigma dz)
__device__ __forceinline__ double ham_cost(double zr, double zi, int dim, int cost_kind, double& sr, double& sim) {
    const double az2 = fma(zr, zr, zi * zi);
    const double rat = (az2 > 1e-300) ? fast_rsqrt(az2) : 0.0;
    const double basic = 1.0 - az2 * rat;   // BasicCost, cost_function.py:140-145
    const bool sq = (cost_kind == 1);       // SquareCost = d / (d + 1) (2 L - L^2) of BasicCost L (cost_function.py:169-173)
    const double dd = dim == 4 ? 0.8 : 8.0 / 9.0;
    const double c0 = sq ? 2.0 * dd : 1.0, c1 = sq ? -dd : 0.0;
    const double fout = basic * fma(c1, basic, c0);
    // sigma = -(d loss / d basic) conj(z) / |z|
    const double dl = fma(2.0 * c1, basic, c0) * rat;
    sr = -dl * zr;
    sim = dl * zi;
    return fout;
}

// The lane's entry of H from its two contributions q = 0, 1: packed indices iw, weights w2[q], parameters xs.  D_q = e^{+-i phi_q} w_q is
// kept: dH[r][c] / ds_q = D_q, dH[r][c] / dphi_q = +-i s_q D_q
struct HamEntry {
    int si[2], pi[2];
    double dr[2], di[2], sv[2], sgn[2];
};
template <bool HUGE_ARGS>
__device__ __forceinline__ void ham_entry(uint32_t iw, const double2* w2, const double* xs, const double2* tbl, HamEntry& e, double& ar, double& ai) {
    ar = 0.0;
    ai = 0.0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint32_t f = iw >> (16 * q);
        e.si[q] = (int)(f & 63u) - 1;
        e.pi[q] = (int)((f >> 6) & 63u) - 1;
        e.sgn[q] = ((f >> 12) & 1u) ? -1.0 : 1.0;
        const double2 w = w2[q];
        e.sv[q] = e.si[q] >= 0 ? xs[e.si[q] >= 0 ? e.si[q] : 0] : 0.0;
        const double ph = e.pi[q] >= 0 ? xs[e.pi[q] >= 0 ? e.pi[q] : 0] : 0.0;
        double s, co;
        if constexpr (HUGE_ARGS) sincos_any(ph, tbl, s, co);
        else sincos_tbl(ph, tbl, s, co);
        s *= e.sgn[q];
        e.dr[q] = fma(co, w.x, -(s * w.y));
        e.di[q] = fma(co, w.y, s * w.x);
        ar = fma(e.sv[q], e.dr[q], ar);
        ai = fma(e.sv[q], e.di[q], ai);
    }
}
// d/ds_q and d/dphi_q of Re(kappa H[r][c]) for the lane's two contributions, kappa = kar + i kai
__device__ __forceinline__ void ham_entry_grad(const HamEntry& e, double kar, double kai, double (&gstr)[2], double (&gphi)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        gstr[q] = fma(kar, e.dr[q], -(kai * e.di[q]));
        gphi[q] = -(e.sgn[q] * e.sv[q]) * fma(kar, e.di[q], kai * e.dr[q]);
    }
}
// what of them goes to parameter j
__device__ __forceinline__ void ham_entry_share(const HamEntry& e, const double (&gstr)[2], const double (&gphi)[2], int j, double& v) {
    v = (e.si[0] == j ? gstr[0] : 0.0) + (e.pi[0] == j ? gphi[0] : 0.0);
    v += (e.si[1] == j ? gstr[1] : 0.0) + (e.pi[1] == j ? gphi[1] : 0.0);
}

// the entry lists into LDS (once per launch); the caller fences
__device__ __forceinline__ void ham_prologue(double* lds, const HamDesc& h) {
    const int lane = threadIdx.x;
    load_sincos_table(reinterpret_cast<double2*>(lds + kQ3OffTbl), lane);
    double2* w = reinterpret_cast<double2*>(lds + kHamOffW);
    w[2 * lane] = reinterpret_cast<const double2*>(h.w)[2 * lane];
    w[2 * lane + 1] = reinterpret_cast<const double2*>(h.w)[2 * lane + 1];
    reinterpret_cast<uint32_t*>(lds + kHamOffIdx)[lane] = h.idx[lane];
    lds_fence();
}

// ---------------------------------------------------------------------------------------------------------------------------
// Fused loss + gradient of one item by the whole wavefront.  In: the trial point in lds[kQ3OffX ..], this lane's target entry
// T[r][c] (zero outside the leading dim x dim block), the entry lists in LDS.  Out: the loss (wave-uniform), the gradient in
// lds[kQ3OffG ..], and with WANT_U this lane's entry of U.
// ---------------------------------------------------------------------------------------------------------------------------
template <bool HUGE_ARGS, bool WANT_U>
__device__ __forceinline__ double eval_ham(double* lds, double tre, double tim, int n, int t_index, int dim, int cost_kind, double& wre,
                                           double& wim) {
    const int lane = threadIdx.x;
    const int r = lane & 7, c = lane >> 3;
    const double2* tbl = reinterpret_cast<const double2*>(lds + kQ3OffTbl);
    const double* xs = lds + kQ3OffX;
    double* gs = lds + kQ3OffG;
    double* lam = lds + kHamOffLam;
    double2* m0 = reinterpret_cast<double2*>(lds + kHamOffM0);
    double2* m1 = reinterpret_cast<double2*>(lds + kHamOffM1);
    double2* m2 = reinterpret_cast<double2*>(lds + kHamOffM2);
    auto sc = [&](double arg, double& s, double& co) {
        if constexpr (HUGE_ARGS) sincos_any(arg, tbl, s, co);
        else sincos_tbl(arg, tbl, s, co);
    };
    // ---- 1. the lane's entry of H
    HamEntry en;
    double ar, ai;
    ham_entry<HUGE_ARGS>(reinterpret_cast<const uint32_t*>(lds + kHamOffIdx)[lane], reinterpret_cast<const double2*>(lds + kHamOffW) + 2 * lane, xs,
                         tbl, en, ar, ai);
    const double t = t_index >= 0 ? xs[t_index >= 0 ? t_index : 0] : 1.0;
    // ---- 2. parallel Jacobi
    double vr = (r == c) ? 1.0 : 0.0, vi = 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kHamMaxSweeps; ++sweep) {
        const double a2 = fma(ar, ar, ai * ai);
        const double off2 = wave_sum(r == c ? 0.0 : a2), all2 = wave_sum(a2);
        if (!(off2 > 1e-30 * all2)) break;  // diagonal to rounding (or not finite: nothing to gain)
        ham_jacobi_step<1>(lds, r, c, ar, ai, vr, vi);
        ham_jacobi_step<2>(lds, r, c, ar, ai, vr, vi);
        ham_jacobi_step<3>(lds, r, c, ar, ai, vr, vi);
        ham_jacobi_step<4>(lds, r, c, ar, ai, vr, vi);
        ham_jacobi_step<5>(lds, r, c, ar, ai, vr, vi);
        ham_jacobi_step<6>(lds, r, c, ar, ai, vr, vi);
        ham_jacobi_step<7>(lds, r, c, ar, ai, vr, vi);
        if (off2 <= 1e-22 * all2) break;  // convergence is quadratic: this sweep has taken it to rounding
    }
    if (r == c) lam[r] = ar;
    m0[r * 8 + c] = make_double2(vr, vi);
    m1[r * 8 + c] = make_double2(tre, tim);
    lds_fence();
    const double lr = lam[r], lc = lam[c];
    // ---- 3. Y = T^+ V, B = V^+ Y, Phi, z
    double yr, yi, br, bi;
    ham_dot8<true, false>(m1 + r, 8, m0 + c, 8, yr, yi);
    m2[r * 8 + c] = make_double2(yr, yi);
    lds_fence();
    ham_dot8<true, false>(m0 + r, 8, m2 + c, 8, br, bi);
    const double hs = 0.5 * t * (lr + lc), hd = 0.5 * t * (lr - lc);
    double sn_s, cs_s, sn_d, cs_d;
    sc(hs, sn_s, cs_s);
    sc(hd, sn_d, cs_d);
    const double snc = ham_sinc(hd, sn_d);
    const double fr = cs_s * snc, fi = -sn_s * snc;  // Phi[r][c]; on the diagonal e_r
    const double qr = fma(br, fr, -(bi * fi)), qi = fma(br, fi, bi * fr);  // (B o Phi)[r][c]
    const double inv_d = dim == 4 ? 0.25 : 0.125;
    const bool diag = r == c;
    const double zr = wave_sum(diag ? qr : 0.0) * inv_d, zi = wave_sum(diag ? qi : 0.0) * inv_d;
    const double ur = wave_sum(diag ? lr * qr : 0.0) * inv_d, ui = wave_sum(diag ? lr * qi : 0.0) * inv_d;  // dz/dt = -i (ur + i ui)
    double sr, sim;
    const double fout = ham_cost(zr, zi, dim, cost_kind, sr, sim);
    if constexpr (WANT_U) {
        double2* ev = reinterpret_cast<double2*>(lds + kHamOffE);
        if (diag) ev[r] = make_double2(fr, fi);
    }
    // ---- 4. K = V (B o Phi) V^+, this lane's K[c][r]
    lds_fence();
    m1[r * 8 + c] = make_double2(qr, qi);
    lds_fence();
    double wr_, wi_, kr, ki;
    ham_dot8<false, true>(m1 + r * 8, 1, m0 + c * 8, 1, wr_, wi_);  // Z[r][c] = sum_b (B o Phi)[r][b] conj(V[c][b])
    m2[r * 8 + c] = make_double2(wr_, wi_);
    lds_fence();
    ham_dot8<false, false>(m0 + c * 8, 1, m2 + r, 8, kr, ki);       // K[c][r] = sum_a V[c][a] Z[a][r]
    if constexpr (WANT_U) {
        const double2* ev = reinterpret_cast<const double2*>(lds + kHamOffE);
        double accr = 0.0, acci = 0.0;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const double2 x = m0[r * 8 + a], y = m0[c * 8 + a], e = ev[a];
            const double pr = fma(x.x, e.x, -(x.y * e.y)), pim = fma(x.x, e.y, x.y * e.x);
            accr = fma(pr, y.x, fma(pim, y.y, accr));
            acci = fma(pim, y.x, fma(-pr, y.y, acci));
        }
        wre = accr;
        wim = acci;
    }
    // kappa = sigma (-i t / d) K[c][r]
    const double mr = t * inv_d * sim, mi = -(t * inv_d * sr);
    const double kar = fma(mr, kr, -(mi * ki)), kai = fma(mr, ki, mi * kr);
    double gstr[2], gphi[2];
    ham_entry_grad(en, kar, kai, gstr, gphi);
    const double gt = fma(sr, ui, sim * ur);  // Re(sigma (-i)(ur + i ui))
    double mine = 0.0;
#pragma unroll 1
    for (int j = 0; j < n; ++j) {
        double v;
        ham_entry_share(en, gstr, gphi, j, v);
        double tot = wave_sum(v);
        if (j == t_index) tot += gt;
        if (lane == j) mine = tot;
    }
    if (lane < n) gs[lane] = mine;
    lds_fence();
    return fout;
}

}  // namespace slamdev
