// slam_analytic.hip -- host side of libslamhip.so, analytic unit: the closed-form decompositions into sqrt(iSWAP) gates
// (slam_analytic.hpp), into gates of the CNOT or the iSWAP class (slam_cx.hpp) and into gates of the B class (slam_b.hpp), and the
// fidelity-aware approximate decomposition into gates of those three classes (slam_approx.hpp), of any supercontrolled class
// (slam_sc.hpp) and into sqrt(iSWAP) gates (slam_sqapprox.hpp).
#include "slam_host.hpp"

#include <complex>
#include <type_traits>

#include "slam_analytic.hpp"
#include "slam_cx.hpp"
#include "slam_b.hpp"
#include "slam_approx.hpp"
#include "slam_sc.hpp"
#include "slam_sqapprox.hpp"

// ---- slam_cx_decompose, slam_b_decompose: the host's share (plain C++) -------------------------------------------------------------------
namespace {

using cd = std::complex<double>;
struct M2 { cd m[2][2]; };
struct M4 { cd m[4][4]; };

M2 load2(const double* p) { return {{{cd(p[0], p[1]), cd(p[2], p[3])}, {cd(p[4], p[5]), cd(p[6], p[7])}}}; }
M2 mul(const M2& a, const M2& b) {
    M2 z;
    for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 2; ++c) z.m[r][c] = a.m[r][0] * b.m[0][c] + a.m[r][1] * b.m[1][c];
    return z;
}
M2 dag(const M2& a) { return {{{std::conj(a.m[0][0]), std::conj(a.m[1][0])}, {std::conj(a.m[0][1]), std::conj(a.m[1][1])}}}; }
M4 kron(const M2& a, const M2& b) {  // a on the high bit
    M4 z;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) z.m[i][j] = a.m[i >> 1][j >> 1] * b.m[i & 1][j & 1];
    return z;
}
M4 mul(const M4& a, const M4& b) {
    M4 z;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            cd s = 0.0;
            for (int k = 0; k < 4; ++k) s += a.m[r][k] * b.m[k][c];
            z.m[r][c] = s;
        }
    return z;
}
// CAN(c): (c1 - c2) sigma_x on span(00, 11) with phase pi/2 c3, (c1 + c2) sigma_x on span(01, 10) with phase -pi/2 c3
M4 can(const double* c) {
    const double hp = 1.57079632679489661923;
    M4 z{};
    const cd e = std::polar(1.0, hp * c[2]), ec = std::conj(e), i1(0.0, 1.0);
    const double am = hp * (c[0] - c[1]), ap = hp * (c[0] + c[1]);
    z.m[0][0] = z.m[3][3] = e * std::cos(am);
    z.m[0][3] = z.m[3][0] = e * i1 * std::sin(am);
    z.m[1][1] = z.m[2][2] = ec * std::cos(ap);
    z.m[1][2] = z.m[2][1] = ec * i1 * std::sin(ap);
    return z;
}
M4 swap_rows(const M4& a) {  // SWAP a
    M4 z = a;
    for (int c = 0; c < 4; ++c) std::swap(z.m[1][c], z.m[2][c]);
    return z;
}
// max |want - e^{i g} got| with the phase that brings them closest; +inf for anything not finite
double phase_distance(const M4& want, const M4& got) {
    cd tr = 0.0;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) tr += std::conj(got.m[r][c]) * want.m[r][c];
    const double n = std::abs(tr);
    if (!(n > 0.0) || !std::isfinite(n)) return INFINITY;
    const cd ph = tr / n;
    double worst = 0.0;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            const double d = std::abs(want.m[r][c] - ph * got.m[r][c]);
            if (!(d <= worst)) worst = d;  // a NaN sticks
        }
    return worst;
}
void put_entry(double* e, const M2& L, const M2& R, int axis, int src) {
    for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 2; ++c) {
            e[2 * (2 * r + c)] = L.m[r][c].real();
            e[2 * (2 * r + c) + 1] = L.m[r][c].imag();
            e[8 + 2 * (2 * r + c)] = R.m[r][c].real();
            e[8 + 2 * (2 * r + c) + 1] = R.m[r][c].imag();
        }
    e[16] = axis;
    e[17] = src;
}

// The head of both dress checks.  dress: n 2x2 factors, the first four l1, l0, r1, r0 (row-major re, im), then the gate's KAK
// coordinates c[3].  Loads the factors into f, checks that c folds onto the class point `own` (`what` names the class in the message)
// and that the first four factors rebuild the gate around CAN(c).
int fold_dress_head(int n, const double* own, const char* what, const double* gate, const double* dress, M2* f) {
    for (int j = 0; j < n; ++j) f[j] = load2(dress + 8 * j);
    const double* c = dress + 8 * n;
    double fc[3] = {c[0], c[1], c[2]};
    if (fc[0] > 0.5) {
        fc[0] = 1.0 - fc[0];
        fc[2] = -fc[2];
    }
    for (int j = 0; j < 3; ++j)
        if (!(std::fabs(std::fabs(fc[j]) - own[j]) < 4e-8))
            return fail(SLAM_ERR_INVALID, "the dress coordinates (%g, %g, %g) are not those of %s", c[0], c[1], c[2], what);
    M4 G;
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) G.m[r][k] = cd(gate[2 * (4 * r + k)], gate[2 * (4 * r + k) + 1]);
    const double d = phase_distance(G, mul(mul(kron(f[0], f[1]), can(c)), kron(f[2], f[3])));
    if (!(d <= 1e-12)) return fail(SLAM_ERR_INVALID, "the dress factors do not rebuild the gate (max deviation %g)", d);
    return SLAM_OK;
}

// Checks gate against dress and folds dress into the kernel's table (slam_cx.hpp).  dress: the twelve 2x2 factors l1, l0, r1, r0,
// a12_1, a12_0, b12_1, b12_0, a21_1, a21_0, b21_1, b21_0 (row-major re, im), then the gate's KAK coordinates c[3].
int cx_fold_dress(int family, const double* gate, const double* dress, double* table) {
    M2 f[12];
    const double own[3] = {0.5, family ? 0.5 : 0.0, 0.0};
    const int rc = fold_dress_head(12, own, family ? "family 1" : "family 0", gate, dress, f);
    if (rc) return rc;
    // D = C or SWAP C with the class point itself; CX12 and CX21 through it
    const M4 C = can(own), D = family ? swap_rows(C) : C;
    M4 cx12{}, cx21{};
    cx12.m[0][0] = cx12.m[1][1] = cx12.m[2][3] = cx12.m[3][2] = 1.0;
    cx21.m[0][0] = cx21.m[2][2] = cx21.m[1][3] = cx21.m[3][1] = 1.0;
    const double tol = 1e-12;
    double d = phase_distance(cx12, mul(mul(kron(f[4], f[5]), D), kron(f[6], f[7])));
    if (!(d <= tol)) return fail(SLAM_ERR_INVALID, "the dress factors do not rebuild CX12 (max deviation %g)", d);
    d = phase_distance(cx21, mul(mul(kron(f[8], f[9]), D), kron(f[10], f[11])));
    if (!(d <= tol)) return fail(SLAM_ERR_INVALID, "the dress factors do not rebuild CX21 (max deviation %g)", d);
    for (int j = 0; j < 32; ++j) table[j] = gate[j];
    // an interior layer K of the D-circuit, qubits (K1, K0): family 1 exchanges the qubits of the first interior layer; then r^+ on the
    // left, l^+ on the right.  Entry order: [slot][qubit 0, qubit 1].
    const M2 l1d = dag(f[0]), l0d = dag(f[1]), r1d = dag(f[2]), r0d = dag(f[3]);
    const M2 &a12_1 = f[4], &a12_0 = f[5], &b12_1 = f[6], &b12_0 = f[7], &a21_1 = f[8], &a21_0 = f[9], &b21_1 = f[10], &b21_0 = f[11];
    double* e = table + 32;
    const int AX = 1, AY = 2, AZ = 3;
    if (!family) {
        // two gates: b12 (RX(a) (x) RZ(b)) a12
        put_entry(e + 0, mul(r0d, b12_0), mul(a12_0, l0d), AZ, 1);
        put_entry(e + 18, mul(r1d, b12_1), mul(a12_1, l1d), AX, 0);
        // three gates, first layer: b12 (RZ(t1) (x) RY(t2)) a21
        put_entry(e + 36, mul(r0d, b12_0), mul(a21_0, l0d), AY, 1);
        put_entry(e + 54, mul(r1d, b12_1), mul(a21_1, l1d), AZ, 0);
    } else {
        put_entry(e + 0, mul(r0d, b12_1), mul(a12_1, l0d), AX, 0);
        put_entry(e + 18, mul(r1d, b12_0), mul(a12_0, l1d), AZ, 1);
        put_entry(e + 36, mul(r0d, b12_1), mul(a21_1, l0d), AZ, 0);
        put_entry(e + 54, mul(r1d, b12_0), mul(a21_0, l1d), AY, 1);
    }
    // three gates, second layer: b21 (1 (x) RY(t3)) a12
    put_entry(e + 72, mul(r0d, b21_0), mul(a12_0, l0d), AY, 2);
    put_entry(e + 90, mul(r1d, b21_1), mul(a12_1, l1d), 0, 0);
    return SLAM_OK;
}

// Checks gate against dress and folds dress into the kernel's table (slam_b.hpp).  dress: the four 2x2 factors l1, l0, r1, r0
// (row-major re, im), then the gate's KAK coordinates c[3].
int b_fold_dress(const double* gate, const double* dress, double* table) {
    M2 f[4];
    const double own[3] = {0.5, 0.25, 0.0};
    const int rc = fold_dress_head(4, own, "the B class (0.5, 0.25, 0)", gate, dress, f);
    if (rc) return rc;
    for (int j = 0; j < 32; ++j) table[j] = gate[j];
    // the interior layer of the G-circuit is r^+ K l^+: qubit 0 first, as the rows hold it
    const M2 order[4] = {dag(f[3]), dag(f[1]), dag(f[2]), dag(f[0])};
    for (int j = 0; j < 4; ++j)
        for (int r = 0; r < 2; ++r)
            for (int k = 0; k < 2; ++k) {
                table[32 + 8 * j + 2 * (2 * r + k)] = order[j].m[r][k].real();
                table[32 + 8 * j + 2 * (2 * r + k) + 1] = order[j].m[r][k].imag();
            }
    return SLAM_OK;
}

// Checks gate against dress and folds dress into the kernel's table (slam_sc.hpp); *beta_p = pi beta / 2 of the gate's class
// (1/2, beta, 0).  dress: the four 2x2 factors l1, l0, r1, r0 (row-major re, im), then the gate's KAK coordinates c[3].  The constant
// matrices of the construction depend on beta alone and are formed here, so a dress cannot carry wrong ones.
int sc_fold_dress(const double* gate, const double* dress, double* table, double* beta_p) {
    M2 f[4];
    const double beta = std::fmin(std::fabs(dress[33]), 0.5);  // a NaN, or anything beyond 1/2, fails the head's check
    const double own[3] = {0.5, beta, 0.0};
    const int rc = fold_dress_head(4, own, "a supercontrolled class (0.5, beta, 0), 0 <= beta <= 0.5", gate, dress, f);
    if (rc) return rc;
    const double bp = 1.57079632679489661923 * beta, h = 0.70710678118654752440;
    const cd i1(0.0, 1.0), em = std::polar(1.0, -bp), ep = std::polar(1.0, bp), Em = std::polar(1.0, -2.0 * bp), Ep = std::polar(1.0, 2.0 * bp);
    const cd p = 1.0 / cd(1.0, 1.0), m = 1.0 / cd(1.0, -1.0);
    const M2 one = {{{1.0, 0.0}, {0.0, 1.0}}};
    const M2 K11l = {{{-p * i1 * em, p * em}, {-p * i1 * ep, -p * ep}}}, K11r = {{{h * i1 * em, -h * em}, {h * ep, -h * i1 * ep}}};
    const M2 K3221l = {{{h * (1.0 + i1 * std::cos(2.0 * bp)), h * i1 * std::sin(2.0 * bp)},
                        {h * i1 * std::sin(2.0 * bp), h * (1.0 - i1 * std::cos(2.0 * bp))}}};
    const M2 K21r = {{{-m * i1 * Em, m * Em}, {m * i1 * Ep, m * Ep}}}, K32r = {{{m * ep, -m * em}, {-m * i1 * ep, -m * i1 * em}}};
    const M2 K22l = {{{h, -h}, {h, h}}}, K22r = {{{0.0, 1.0}, {-1.0, 0.0}}}, ipz = {{{i1, 0.0}, {0.0, -i1}}};
    for (int j = 0; j < 32; ++j) table[j] = gate[j];
    // an interior factor L rz(t) R of the S-circuit is (r^+ L) rz(t) (R l^+) in the G-circuit; entry order as slam_sc.hpp lists it
    const M2 l1d = dag(f[0]), l0d = dag(f[1]), r1d = dag(f[2]), r0d = dag(f[3]);
    const M2 L[kScEntries] = {mul(r0d, mul(ipz, dag(K11r))), mul(r1d, dag(K11l)), mul(r0d, K22r), mul(r1d, K22l), mul(r0d, K32r),
                              mul(r1d, mul(K3221l, l1d))};
    const M2 R[kScEntries] = {mul(K11r, l0d), mul(K11l, l1d), mul(K11r, l0d), mul(K11l, l1d), mul(K21r, l0d), one};
    for (int j = 0; j < kScEntries; ++j)
        for (int r = 0; r < 2; ++r)
            for (int k = 0; k < 2; ++k) {
                double* e = table + 32 + 16 * j + 2 * (2 * r + k);
                e[0] = L[j].m[r][k].real();
                e[1] = L[j].m[r][k].imag();
                e[8] = R[j].m[r][k].real();
                e[9] = R[j].m[r][k].imag();
            }
    *beta_p = bp;
    return SLAM_OK;
}

// an argument block with a third double per target, `predicted` (slam_approx.hpp)
template <class Args, class = void>
struct has_predicted : std::false_type {};
template <class Args>
struct has_predicted<Args, std::void_t<decltype(std::declval<Args&>().predicted)>> : std::true_type {};

// What the entry points do once their own arguments are checked: the context and the window, the buffers, the kernel's table
// (n_table doubles, the gate and the interior factors; none for sqrt(iSWAP)) into ev_x, the launch and the read-backs, any of which
// may be NULL.  `own` fills the fields that only this family's argument block has, given the table's device address.
template <class Args, class Own>
int run_closed_form(slam_ctx* ctx, int64_t first, int64_t count, void (*kernel)(Args), const double* table, size_t n_table, Own own,
                    double* x_out, int32_t* cycles, double* loss, double* gap, double* predicted = nullptr) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (first < 0 || count < 0 || first + count > ctx->n_targets)
        return fail(SLAM_ERR_INVALID, "target window outside the resident batch");
    if (count > 0x7fffffffLL) return fail(SLAM_ERR_INVALID, "too many targets in one call (%lld)", (long long)count);
    if (count == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->ev_grad.reserve((size_t)count * 24 * sizeof(double)));  // the rows
    constexpr size_t per_target = has_predicted<Args>::value ? 3 : 2;
    HIP_TRY(ctx->ev_loss.reserve((size_t)count * per_target * sizeof(double)));  // losses, then gaps (then predicted losses)
    HIP_TRY(ctx->ev_tof.reserve((size_t)count * sizeof(int32_t)));       // sizes
    if (table) {
        HIP_TRY(ctx->ev_x.reserve(n_table * sizeof(double)));
        HIP_TRY(hipMemcpy(ctx->ev_x.p, table, n_table * sizeof(double), hipMemcpyHostToDevice));  // from the caller's stack: done before the call goes on
    }
    Args a{};
    own(a, ctx->ev_x.as<double>());
    a.targets = ctx->targets.as<double>() + first * 32;
    a.M = count;
    a.x_out = ctx->ev_grad.as<double>();
    a.cycles = ctx->ev_tof.as<int32_t>();
    a.loss = ctx->ev_loss.as<double>();
    a.gap = ctx->ev_loss.as<double>() + count;
    if constexpr (has_predicted<Args>::value) a.predicted = ctx->ev_loss.as<double>() + 2 * count;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((count + kKakBlock - 1) / kKakBlock)), dim3(kKakBlock), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    if (x_out) HIP_TRY(hipMemcpyAsync(x_out, a.x_out, (size_t)count * 24 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (cycles) HIP_TRY(hipMemcpyAsync(cycles, a.cycles, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (loss) HIP_TRY(hipMemcpyAsync(loss, a.loss, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (gap) HIP_TRY(hipMemcpyAsync(gap, a.gap, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if constexpr (has_predicted<Args>::value)
        if (predicted) HIP_TRY(hipMemcpyAsync(predicted, a.predicted, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

// The family's table for the approximate kernels: the gate and the interior factors, checked and folded as the exact siblings do.
int approx_table(int family, const double* gate, const double* dress, double* table, size_t* n_table) {
    if (family < 0 || family > 2)
        return fail(SLAM_ERR_INVALID, "family must be 0 (CNOT class), 1 (iSWAP class) or 2 (B class), got %d", family);
    if (!gate || !dress) return fail(SLAM_ERR_INVALID, "gate and dress are required");
    *n_table = family == 2 ? kBTable : kCxTable;
    return family == 2 ? b_fold_dress(gate, dress, table) : cx_fold_dress(family, gate, dress, table);
}

// What the two sweeps do once the gate is known: the fidelities and the window are checked, the outputs cleared, the fidelities
// uploaded, the histogram zeroed, the launch and the two optional read-backs.  `own` fills what only this kernel's block has.
template <class Args, class Own>
int run_counts(slam_ctx* ctx, int64_t first, int64_t count, void (*kernel)(Args), Own own, int32_t n_fid, const double* fidelities,
               int64_t* counts_out, int64_t* fidsum_out) {
    if (n_fid < 1 || n_fid > kApproxMaxFid) return fail(SLAM_ERR_INVALID, "n_fid must be in 1..%d, got %d", kApproxMaxFid, n_fid);
    if (!fidelities) return fail(SLAM_ERR_INVALID, "fidelities is NULL");
    for (int32_t j = 0; j < n_fid; ++j)
        if (!(fidelities[j] > 0.0 && fidelities[j] <= 1.0))
            return fail(SLAM_ERR_INVALID, "fidelities[%d] must be in (0, 1], got %g", j, fidelities[j]);
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (first < 0 || count < 0 || first + count > ctx->n_targets)
        return fail(SLAM_ERR_INVALID, "target window outside the resident batch");
    if (count > 0x7fffffffLL) return fail(SLAM_ERR_INVALID, "too many targets in one call (%lld)", (long long)count);
    if (counts_out) std::memset(counts_out, 0, (size_t)n_fid * 4 * sizeof(int64_t));
    if (fidsum_out) std::memset(fidsum_out, 0, (size_t)n_fid * sizeof(int64_t));
    if (count == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->ev_x.reserve((size_t)n_fid * sizeof(double)));
    HIP_TRY(ctx->ev_loss.reserve((size_t)n_fid * 5 * sizeof(unsigned long long)));  // counts [n_fid][4], then sums [n_fid]
    HIP_TRY(hipMemcpy(ctx->ev_x.p, fidelities, (size_t)n_fid * sizeof(double), hipMemcpyHostToDevice));  // the caller's array: done before the call goes on
    HIP_TRY(hipMemsetAsync(ctx->ev_loss.p, 0, (size_t)n_fid * 5 * sizeof(unsigned long long), ctx->stream));
    Args a{};
    own(a);
    a.targets = ctx->targets.as<double>() + first * 32;
    a.fidelities = ctx->ev_x.as<double>();
    a.M = count;
    a.n_fid = n_fid;
    a.counts = ctx->ev_loss.as<unsigned long long>();
    a.fidsum = a.counts + (size_t)n_fid * 4;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((count + kApproxCountsBlock - 1) / kApproxCountsBlock)), dim3(kApproxCountsBlock), 0,
                       ctx->stream, a);
    HIP_TRY(hipGetLastError());
    if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, a.counts, (size_t)n_fid * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (fidsum_out) HIP_TRY(hipMemcpyAsync(fidsum_out, a.fidsum, (size_t)n_fid * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

}  // namespace

extern "C" {

// Gate, dress and family are checked before the context -- what needs no context first: the host's share runs, and is checked, on a
// machine without a device too.
int slam_b_decompose(slam_ctx* ctx, int64_t first, int64_t count, const double* gate, const double* dress, double* x_out, int32_t* cycles,
                     double* loss, double* gap) {
    if (!gate || !dress) return fail(SLAM_ERR_INVALID, "gate and dress are required");
    double table[kBTable];
    const int rc = b_fold_dress(gate, dress, table);
    if (rc) return rc;
    return run_closed_form(ctx, first, count, b_decompose_kernel, table, kBTable, [](BArgs& a, const double* t) { a.table = t; }, x_out, cycles, loss, gap);
}

int slam_cx_decompose(slam_ctx* ctx, int64_t first, int64_t count, int family, const double* gate, const double* dress, double* x_out,
                      int32_t* cycles, double* loss, double* gap) {
    if (family != 0 && family != 1) return fail(SLAM_ERR_INVALID, "family must be 0 (CNOT class) or 1 (iSWAP class), got %d", family);
    if (!gate || !dress) return fail(SLAM_ERR_INVALID, "gate and dress are required");
    double table[kCxTable];
    const int rc = cx_fold_dress(family, gate, dress, table);
    if (rc) return rc;
    return run_closed_form(
        ctx, first, count, cx_decompose_kernel, table, kCxTable, [family](CxArgs& a, const double* t) { a.table = t, a.family = family; }, x_out,
        cycles, loss, gap);
}

int slam_sqiswap_decompose(slam_ctx* ctx, int64_t first, int64_t count, double* x_out, int32_t* cycles, double* loss, double* gap) {
    return run_closed_form(ctx, first, count, sqiswap_decompose_kernel, nullptr, 0, [](AnalyticArgs&, const double*) {}, x_out, cycles, loss, gap);
}

int slam_approx_decompose(slam_ctx* ctx, int64_t first, int64_t count, int family, const double* gate, const double* dress,
                          double basis_fidelity, int force_cycles, double* x_out, int32_t* cycles, double* loss, double* predicted,
                          double* gap) {
    static_assert(kCxTable >= kBTable, "one table buffer for the three families");
    double table[kCxTable];
    size_t n_table = 0;
    const int rc = approx_table(family, gate, dress, table, &n_table);
    if (rc) return rc;
    if (!(basis_fidelity > 0.0 && basis_fidelity <= 1.0))  // a NaN fails both
        return fail(SLAM_ERR_INVALID, "basis_fidelity must be in (0, 1], got %g", basis_fidelity);
    const int k_max = family == 2 ? 2 : 3;
    if (force_cycles < -1 || force_cycles > k_max)
        return fail(SLAM_ERR_INVALID, "force_cycles must be -1 (select) or 0..%d for family %d, got %d", k_max, family, force_cycles);
    return run_closed_form(
        ctx, first, count, approx_decompose_kernel, table, n_table,
        [=](ApproxArgs& a, const double* t) { a.table = t, a.family = family, a.force = force_cycles, a.fidelity = basis_fidelity; }, x_out,
        cycles, loss, gap, predicted);
}

int slam_approx_counts(slam_ctx* ctx, int64_t first, int64_t count, int family, int32_t n_fid, const double* fidelities,
                       int64_t* counts_out, int64_t* fidsum_out) {
    if (family < 0 || family > 2)
        return fail(SLAM_ERR_INVALID, "family must be 0 (CNOT class), 1 (iSWAP class) or 2 (B class), got %d", family);
    return run_counts(ctx, first, count, approx_counts_kernel, [family](ApproxCountsArgs& a) { a.family = family; }, n_fid, fidelities,
                      counts_out, fidsum_out);
}

int slam_sc_decompose(slam_ctx* ctx, int64_t first, int64_t count, const double* gate, const double* dress, double basis_fidelity,
                      int force_cycles, double* x_out, int32_t* cycles, double* loss, double* predicted, double* gap) {
    if (!gate || !dress) return fail(SLAM_ERR_INVALID, "gate and dress are required");
    double table[kScTable], bp = 0.0;
    const int rc = sc_fold_dress(gate, dress, table, &bp);
    if (rc) return rc;
    if (!(basis_fidelity > 0.0 && basis_fidelity <= 1.0))  // a NaN fails both
        return fail(SLAM_ERR_INVALID, "basis_fidelity must be in (0, 1], got %g", basis_fidelity);
    if (force_cycles < -1 || force_cycles > 3)
        return fail(SLAM_ERR_INVALID, "force_cycles must be -1 (select) or 0..3, got %d", force_cycles);
    return run_closed_form(
        ctx, first, count, sc_decompose_kernel, table, kScTable,
        [=](ScArgs& a, const double* t) { a.table = t, a.beta_p = bp, a.force = force_cycles, a.fidelity = basis_fidelity; }, x_out, cycles,
        loss, gap, predicted);
}

int slam_sc_counts(slam_ctx* ctx, int64_t first, int64_t count, const double* gate, const double* dress, int32_t n_fid,
                   const double* fidelities, int64_t* counts_out, int64_t* fidsum_out) {
    if (!gate || !dress) return fail(SLAM_ERR_INVALID, "gate and dress are required");
    double table[kScTable], bp = 0.0;
    const int rc = sc_fold_dress(gate, dress, table, &bp);
    if (rc) return rc;
    return run_counts(ctx, first, count, sc_counts_kernel, [bp](ScCountsArgs& a) { a.beta_p = bp; }, n_fid, fidelities, counts_out,
                      fidsum_out);
}

int slam_sqiswap_approx_decompose(slam_ctx* ctx, int64_t first, int64_t count, double basis_fidelity, int force_cycles, double* x_out,
                                  int32_t* cycles, double* loss, double* predicted, double* gap) {
    if (!(basis_fidelity > 0.0 && basis_fidelity <= 1.0))  // a NaN fails both
        return fail(SLAM_ERR_INVALID, "basis_fidelity must be in (0, 1], got %g", basis_fidelity);
    if (force_cycles < -1 || force_cycles > 3)
        return fail(SLAM_ERR_INVALID, "force_cycles must be -1 (select) or 0..3, got %d", force_cycles);
    return run_closed_form(
        ctx, first, count, sqiswap_approx_decompose_kernel, nullptr, 0,
        [=](SqApproxArgs& a, const double*) { a.force = force_cycles, a.fidelity = basis_fidelity; }, x_out, cycles, loss, gap, predicted);
}

int slam_sqiswap_approx_counts(slam_ctx* ctx, int64_t first, int64_t count, int32_t n_fid, const double* fidelities, int64_t* counts_out,
                               int64_t* fidsum_out) {
    return run_counts(ctx, first, count, sqiswap_approx_counts_kernel, [](SqApproxCountsArgs&) {}, n_fid, fidelities, counts_out, fidsum_out);
}

}  // extern "C"
