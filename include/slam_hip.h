/*
 * slam_hip.h -- C ABI of libslamhip.so, the MI355X (gfx950) implementation of the
 * SLAM template-optimizer inner loop.
 *
 * The reference (Pitt-JonesLab/slam_decomposition) is pure Python: there is no FFI
 * today.  Each entry point below states the reference code it replaces
 * (paths relative to the reference checkout).  Python binds these with ctypes
 * (slam_decomposition_amd/_ffi.py); INTEGRATION.md shows the stub a maintainer of
 * the reference would add to src/slam/optimizer.py.
 *
 * Conventions
 *   - plain pointers and sizes only; every buffer is caller-allocated, C-contiguous,
 *     8-byte aligned host memory; the library never keeps a caller pointer after
 *     the call returns.  Device buffers are owned by the context.
 *   - complex matrices are row-major interleaved (re, im) doubles: a 4x4 matrix is
 *     double[4][4][2] = 32 doubles.
 *   - template parameters x are in index order P0..P{n-1}, n = 6(k+1): layer-major,
 *     within a layer (theta, phi, lambda) of the qubit-0 U gate then of the qubit-1
 *     U gate  (reference: src/slam/basis.py:152-169).
 *   - functions return 0 on success or a negative SLAM_ERR_* code;
 *     slam_last_error() gives the message for the calling thread.
 *   - one context = one GPU = one host thread at a time.  Multi-GPU = one context
 *     per device, one process per GPU, merged through slam_comm_* (RCCL) at the end.
 */
#ifndef SLAM_HIP_H
#define SLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_OK 0
#define SLAM_ERR_INVALID (-1)     /* bad argument */
#define SLAM_ERR_HIP (-2)         /* HIP runtime error (message has the HIP string) */
#define SLAM_ERR_UNSUPPORTED (-3) /* e.g. span outside [1, SLAM_MAX_SPAN_MINIMIZE] */
#define SLAM_ERR_NOMEM (-4)
#define SLAM_ERR_STATE (-5)       /* call order: targets / basis not set */

#define SLAM_MAX_SPAN_QUAD 5      /* spans of the register-resident kernels (a quad of lanes per item; 1..3 are the tuned ones);
                                    the reference's default maximum_span_guess, src/slam/basis.py:59 */
#define SLAM_MAX_SPAN_EVAL 16     /* spans of slam_eval_*: beyond SLAM_MAX_SPAN_QUAD one wavefront per item (csrc/slam_long.hpp) */
#define SLAM_MAX_SPAN_MINIMIZE 16 /* spans of slam_minimize_stage / slam_decompose*: beyond SLAM_MAX_SPAN_QUAD a wavefront per item
                                    with its quasi-Newton metric (fp32) in device memory (the templates MixedOrderBasisCircuitTemplate builds from
                                    weak gates, src/slam/basis.py:213-359) */
#define SLAM_MAX_GATES 256
#define SLAM_MAX_MAXITER 4000    /* per-restart iteration cap accepted by the kernels (reference: 2500) */

/* per-item optimizer status (slam_minimize_stage: item_status) */
#define SLAM_ST_CONVERGED 0 /* loss < stop_loss or |g|_inf < gtol */
#define SLAM_ST_MAXITER 1   /* reference: options={"maxiter": 2500}, src/slam/optimizer.py:275 */
#define SLAM_ST_LINESEARCH 2
#define SLAM_ST_NONFINITE 3
#define SLAM_ST_STALLED 4   /* no representable decrease (fp64 noise floor at a non-zero minimum) */
#define SLAM_ST_PREEMPTED 5 /* a sibling restart of the same target reached stop_loss first
                               (reference: break over restarts, src/slam/optimizer.py:287-295) */

/* flags for slam_minimize_stage / slam_decompose */
#define SLAM_FLAG_EARLY_EXIT 1u /* stop a target's other restarts once one reaches stop_loss */
#define SLAM_FLAG_ORDERED 2u    /* with EARLY_EXIT: a successful restart (final loss < the span loop's success threshold;
                                   stop_loss in slam_minimize_stage) only stops the restarts with a HIGHER index, and the
                                   stage result is the lowest-index successful restart -- exactly the restart at which
                                   the reference's sequential loop breaks (src/slam/optimizer.py:287-295).  Results are
                                   then independent of scheduling, shard layout and items_per_quad (bitwise
                                   reproducible for a fixed seed); without it the first restart to FINISH wins, which
                                   runs fewer evaluations but depends on timing. */
#define SLAM_FLAG_STAGED 4u     /* span loops (slam_decompose*): always one optimizer launch + one bookkeeping launch per span.
                                   Without it a SMALL batch (at most one target per SIMD, at most 16 restarts -- or up to 64
                                   when targets x restarts fill the chip --, spans <= 3, ordered early exit, one gate structure
                                   class) runs through the one-wavefront-per-target kernel: a single launch in
                                   which every target goes from span to span on its own -- same items, same seeds, same
                                   results bit for bit, no stage barrier (round 4).  It also forces the span-by-span order
                                   where calls of at most two targets per CU (speculative spans) and calls of at most 2^17
                                   work items per span (overlapped spans) would run their spans side by side. */
#define SLAM_FLAG_OVERLAP 8u    /* span loops: run the spans side by side for ALL targets of the call whatever its size -- one
                                   optimizer launch per span on its own stream, the loop's bookkeeping afterwards in span order.
                                   Same results bit for bit; the stages the loop would not have reached are wasted work, so this
                                   pays when the early spans cannot succeed anyway (a CNOT basis: no generic target before three
                                   gates) and the call is alone on the device.  Needs EARLY_EXIT | ORDERED, spans <= 3. */
#define SLAM_FLAG_NO_OVERLAP 16u /* span loops: never run the spans of a MEDIUM call (at most 2^17 work items per span) side by side,
                                   which the library does by itself otherwise -- for callers that keep several calls in flight on
                                   the device: the chip is full then and the speculative stages only add work. */

#define SLAM_FLAG_NO_EXTERIOR 32u /* fixed-gate templates: CircuitTemplate(no_exterior_1q=True), src/slam/basis.py:57,154,165 -- the
                                   template is G_k K_{k-1} ... K_1 G_1: the six parameters of layer 0 and of layer k are pinned at zero
                                   (U3(0, 0, 0) = 1; start values and gradient components zeroed), so the optimisation runs over the
                                   6 (k - 1) interior parameters; x rows keep the 6 (k + 1) layout with zeros in the pinned places. */

typedef struct slam_ctx slam_ctx;

typedef struct slam_opt_params {
    int32_t restarts;     /* R: multi-start seeds per target per span (TRAINING_RESTARTS, optimizer.py:19) */
    int32_t maxiter;      /* per-restart iteration cap (optimizer.py:275: 2500) */
    double gtol;          /* stop when |g|_inf < gtol (SciPy BFGS default 1e-5; we default 1e-9) */
    double stop_loss;     /* stop when loss < stop_loss */
    uint64_t seed;        /* Philox key for x0 ~ U[0,2pi)^n (basis.py:106-111) */
    uint32_t flags;       /* SLAM_FLAG_* (bits above SLAM_FLAG_ORDERED are ignored) */
    uint32_t items_per_quad; /* launch shaping: at least this many work items per resident quad before more
                                wavefronts are launched.  0/1 = spread a small batch over as many wavefronts as
                                possible (lowest latency of one batch); 4..8 = keep quads refilled (highest
                                throughput when several batches are in flight on different streams).  With
                                SLAM_FLAG_ORDERED (or without early exit) results do not depend on it; with the plain
                                early-exit flag the winner among equally successful restarts depends on timing anyway. */
    double gtol_far;      /* with far_loss: also stop when |g|_inf < gtol_far and loss > far_loss, i.e. at a */
    double far_loss;      /* stationary point that is clearly not a zero of the loss.  gtol_far = 1e-5 is SciPy's
                             default gtol, which is what the reference runs with (optimizer.py:270-278);
                             set gtol_far = 0 to disable */
    int64_t target_base;  /* added to a target's index within the context's resident batch in the Philox key, so that a
                             shard holding targets [base, base + n) of a larger job draws the seeds the whole job would */
} slam_opt_params;

typedef struct slam_stats {
    double kernel_ms;         /* sum of HIP-event durations of the minimize kernel launches */
    int64_t kernel_launches;  /* number of minimize kernel launches */
    int64_t evals[SLAM_MAX_SPAN_EVAL + 1]; /* fused loss+grad evaluations per span k (index k) */
    int64_t items[SLAM_MAX_SPAN_EVAL + 1]; /* (target, seed) work items per span k */
    double total_ms;          /* HIP-event time of the last slam_decompose / slam_minimize_stage */
    double kernel_ms_span[SLAM_MAX_SPAN_EVAL + 1]; /* per span k (index k >= 1): HIP-event time of span k's optimizer launches.  Span-by-span
                                                      calls: they add up to kernel_ms.  Calls that run their spans side by side
                                                      (speculative / overlapped spans): each span's own launch -- overlapping in time, so
                                                      their sum exceeds kernel_ms.  Index 0: time of launches that cover SEVERAL spans (the
                                                      one-wavefront-per-target loop), for which no per-span split exists. */
    int64_t wave_rounds[SLAM_MAX_SPAN_EVAL + 1];   /* lock-step evaluation rounds summed over wavefronts, per span:
                                                      evals / (16 * wave_rounds) = fraction of quads that held an item */
    /* split of evals[k]: evaluations whose point was accepted (a restart's initial point or an Armijo-accepted
       step), evaluations of restarts that ended pre-empted by a successful sibling (all of them, accepted or not);
       the rest, evals - accepted - preempted, are rejected line-search trials */
    int64_t evals_accepted[SLAM_MAX_SPAN_EVAL + 1];
    int64_t evals_preempted[SLAM_MAX_SPAN_EVAL + 1];
} slam_stats;

/* Thread-local message of the last failing call on this thread. */
const char* slam_last_error(void);

/* Number of visible HIP devices. */
int slam_device_count(int* count);

/* Create / destroy a context bound to one device.  Creates a private HIP stream. */
int slam_ctx_create(int device, slam_ctx** out);
int slam_ctx_destroy(slam_ctx* ctx);

/* Name and CU count of the context's device (name buffer >= 256 bytes). */
int slam_ctx_device_info(slam_ctx* ctx, char* name, int name_len, int* compute_units, int* clock_khz);

/*
 * Upload the batch of target unitaries (resident in HBM until replaced).
 * Replaces iterating the sampler one target at a time:
 *   src/slam/optimizer.py:180-186 (approximate_from_distribution), src/slam/sampler.py:25-27.
 * targets: double[n_targets][4][4][2].
 */
int slam_set_targets(slam_ctx* ctx, const double* targets, int64_t n_targets);

/*
 * Fill the resident batch with n_targets Haar-random 4x4 unitaries generated on the device:
 * T_i = QR(Ginibre(Philox(seed, first_index + i))).Q with a positive diagonal of R -- the recipe of
 * HaarSample._get_unitary (src/slam/sampler.py:62-71 -> qiskit random_unitary -> SciPy unitary_group),
 * with Philox4x32-10 + Box-Muller in place of NumPy's generator: same distribution, different sample.
 * slam_get_targets copies resident targets [first, first + count) back: double[count][4][4][2].
 */
int slam_sample_haar(slam_ctx* ctx, uint64_t seed, int64_t first_index, int64_t n_targets);
int slam_get_targets(slam_ctx* ctx, int64_t first, int64_t count, double* out);

/*
 * The same generator for an explicit list of stream indices: T_i = Haar(seed, indices[i]) becomes the resident batch (it replaces
 * the resident targets like slam_sample_haar).  indices: host memory, int64[n_targets], each >= 0, any order, repeats allowed.
 * slam_sample_haar_indexed(seed, {s, s + 1, ..}) gives the bits of slam_sample_haar(seed, s, ..).
 */
int slam_sample_haar_indexed(slam_ctx* ctx, uint64_t seed, const int64_t* indices, int64_t n_targets);

/*
 * Haar targets of a known template size, selected on the device: Haar2Sample / Haar3Sample (src/slam/sampler.py:73-107: draw, run the
 * analytic sqrt(iSWAP) pass, count its gates, discard on a mismatch) for any gate sequence.  Every candidate i of
 * [first_index, first_index + n_candidates) gets the unitary of slam_sample_haar(seed, i) and the span of slam_predict_spans for the
 * half-spaces `point`, `bounds[k_max][14]`, `tol` (0 local, 1 .. k_max, k_max + 1 out of reach), both in registers: a rejected
 * candidate costs no memory traffic.  A candidate is selected when span_lo <= span <= span_hi and, with margin > 0, when it gets the
 * same span with tol + margin and with tol - margin (it is clear of every region boundary by `margin`, units of pi).
 *   n_selected   the number of selected candidates of the whole range (may exceed capacity)
 *   indices_out  host memory, int64[capacity]: the stream indices of the first min(*n_selected, capacity) selected candidates in
 *                increasing order -- ranks come from ballots and prefix sums, never from an atomic, so the list depends on the
 *                arguments alone; feed it to slam_sample_haar_indexed
 *   span_counts  optional, host memory, int64[k_max + 2]: ADDED TO with the number of scanned candidates per span at the plain tol
 *                (their shares are the Haar volumes of the prefix regions)
 * The resident targets are not touched.  n_candidates <= 2^31 - 1 per call, 0 <= span_lo <= span_hi <= k_max + 1, margin >= 0.
 */
int slam_haar_select_spans(slam_ctx* ctx, uint64_t seed, int64_t first_index, int64_t n_candidates, int k_max, const double* point,
                           const double* bounds, double tol, double margin, int32_t span_lo, int32_t span_hi, int64_t capacity,
                           int64_t* n_selected, int64_t* indices_out, int64_t* span_counts);

/*
 * Weyl-chamber coordinates (c1, c2, c3), in units of pi, of 4x4 unitaries -- weylchamber.c1c2c3 as called by
 * VariationalTemplate.target_invariant (src/slam/basis_abc.py:80-84) and on the optimizer's results
 * (src/slam/optimizer.py:85,103,224) -- computed on the device, one thread per unitary.  ndigits >= 0 rounds like
 * numpy.round (the reference uses 8); ndigits < 0 leaves the values unrounded.  out: double[count][3].
 *   slam_c1c2c3          unitaries from the host, double[count][4][4][2]
 *   slam_targets_c1c2c3  the resident targets [first, first + count) (nothing is uploaded)
 *   slam_eval_c1c2c3     the template unitaries CircuitTemplate.eval(x[m]) of M parameter vectors (the unitaries
 *                        stay on the device; needs resident targets and gates like slam_eval_unitary)
 */
int slam_c1c2c3(slam_ctx* ctx, const double* unitaries, int64_t count, int ndigits, double* out);
int slam_targets_c1c2c3(slam_ctx* ctx, int64_t first, int64_t count, int ndigits, double* out);
int slam_eval_c1c2c3(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x, int64_t M, int ndigits, double* out);

/*
 * KAK decomposition on the device, one thread per unitary (csrc/slam_kak.hpp):
 *     U = e^{i phase} (a1 (x) a2) CAN(c) (b1 (x) b2),   CAN(c) = exp(i pi/2 (c1 XX + c2 YY + c3 ZZ)),
 * with a1, a2, b1, b2 in SU(2) (index 1: the qubit of the high bit of the basis index, qiskit's qubit 1) and c, in units of pi, the
 * chamber point slam_c1c2c3 returns with ndigits < 0 (same fold, same c3 < 0 -> (1 - c1, c2, -c3) rule).  The reference has no such
 * step of its own: its transpiler pass calls qiskit's KAK code, and VariationalTemplate.undo_invariant_transform
 * (src/slam/basis_abc.py:86-90) is a stub.
 *   phase double[count], a1 / a2 / b1 / b2 double[count][2][2][2], c double[count][3]   (out, all required)
 *   slam_kak          unitaries from the host, double[count][4][4][2]
 *   slam_targets_kak  the resident targets [first, first + count) (nothing is uploaded)
 *
 * slam_complete_locals: local-gate completion of M fits that hold up to single-qubit gates (MakhlinFunctionalCost, or
 * SLAM_FLAG_NO_EXTERIOR templates).  Item m: W = template(x[m]) (gate_seq, k as in slam_eval_unitary; rows of no-exterior fits carry
 * zeros in layers 0 and k), T = resident target target_of[m].  KAK of both, the chamber points aligned (the c3 = 0 mirror image
 * (1 - c1, c2, -c3) of W's point is taken where it is closer to T's), L = A_T A_W^+ folded into layer k and R = B_W^+ B_T into layer 0:
 *   x_out     double[M][6(k+1)]  the completed row; interior layers are copied
 *   loss_out  double[M]          1 - |Tr(T^+ template(x_out))| / 4, from a forward pass of x_out
 *   gap_out   double[M]          max-norm distance d of the two chamber points after alignment (units of pi); loss <= 1 - cos(1.5 pi d)
 */
int slam_kak(slam_ctx* ctx, const double* unitaries, int64_t count, double* phase, double* a1, double* a2, double* c, double* b1, double* b2);
int slam_targets_kak(slam_ctx* ctx, int64_t first, int64_t count, double* phase, double* a1, double* a2, double* c, double* b1, double* b2);
int slam_complete_locals(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x, const int32_t* target_of, int64_t M, double* x_out,
                         double* loss_out, double* gap_out);

/*
 * Closed-form decomposition into sqrt(iSWAP) gates on the device, one thread per resident target (csrc/slam_analytic.hpp; Huang et
 * al., arXiv:2105.06074; the reference's RootiSwapWeylDecomposition.riswapWeylDecomp,
 * src/slam/utils/transpiler_pass/weyl_decompose.py:343-449): no optimiser, no restarts, no gate table -- the basis gate is
 * S = RiSwapGate(1/2) = exp(i pi/8 (XX + YY)).  For the resident targets [first, first + count) (nothing is uploaded):
 *   x_out   double[count][24]  the 6 (k + 1) template angles in the index order of slam_eval_unitary in the front of the row, zeros
 *                              behind; layers 0 and k are the exterior: template(x, [S] * k) = e^{i phi} T
 *   cycles  int32[count]       k: 2 iff |z| <= x - y + 2e-8 on the coordinates rounded to 8 digits and folded to c1 <= 1/2
 *                              (span_rules.minimal_span; what slam_predict_spans says with tol = 2e-8), else 3
 *   loss    double[count]      1 - |Tr(T^+ template(x_out))| / 4, from a forward pass of the written row
 *   gap     double[count]      max-norm distance (units of pi) that remains between the chamber points when the interior two-gate
 *                              circuit is aligned with the class it was built for, as slam_complete_locals' gap_out:
 *                              loss <= 1 - cos(1.5 pi gap)
 * Like the reference's pass the function returns 2 or 3 gates only: a local target and a target of S's own class get a valid
 * two-gate circuit.  Any output pointer may be NULL.  SLAM_ERR_INVALID for a window outside the resident batch.
 */
int slam_sqiswap_decompose(slam_ctx* ctx, int64_t first, int64_t count, double* x_out, int32_t* cycles, double* loss, double* gap);

/*
 * Closed-form decomposition into one, two or three gates G of the CNOT class (family 0: CX, CZ, ...) or of the iSWAP class (family 1) on
 * the device, one thread per resident target (csrc/slam_cx.hpp; Vatan and Williams, quant-ph/0308006; the TwoQubitBasisDecomposer
 * branch of the reference's pass, src/slam/utils/transpiler_pass/weyl_decompose.py:475-480).  The interior angles are linear in the
 * target's KAK coordinates.  For the resident targets [first, first + count) (nothing is uploaded, no gate table is needed):
 *   gate    double[32]         G, row-major (re, im)
 *   dress   double[SLAM_CX_DRESS]  the host's reduction of G: twelve 2x2 factors (row-major re, im; in a pair the factor of the qubit of
 *                              the high bit comes first) l1, l0, r1, r0, a12_1, a12_0, b12_1, b12_0, a21_1, a21_0, b21_1, b21_0, then
 *                              c[3], with  G = e^{i .} (l1 (x) l0) CAN(c) (r1 (x) r0),  c the KAK coordinates of G (within 4e-8 of the
 *                              family's class point C = (1/2, 0, 0) or (1/2, 1/2, 0)), and with D = CAN(C) (family 0) or SWAP CAN(C)
 *                              (family 1):  CX12 = e^{i .} (a12_1 (x) a12_0) D (b12_1 (x) b12_0),  CX21 likewise with a21, b21
 *                              (CX12 = |0><0| (x) 1 + |1><1| (x) X, CX21 = 1 (x) |0><0| + X (x) |1><1|)
 *   x_out   double[count][24]  the 6 (k + 1) template angles in the index order of slam_eval_unitary in the front of the row, zeros
 *                              behind: template(x, [G] * k) = e^{i phi} T
 *   cycles  int32[count]       k: on the coordinates rounded to 8 digits and folded to c1 <= 1/2 (span_rules.minimal_span, tolerance
 *                              2e-8) 1 in G's own class, else 2 where |c3| < 2e-8, else 3; a local target gets two gates
 *   loss    double[count]      1 - |Tr(T^+ template(x_out))| / 4, from a forward pass of the written row
 *   gap     double[count]      max-norm distance (units of pi) that remains between the chamber points when the interior circuit is
 *                              aligned with the target, as slam_complete_locals' gap_out: rounding only for three gates
 * Any output pointer may be NULL.  SLAM_ERR_INVALID for a NULL context, a window outside the resident batch, an unknown family, and
 * a gate that the dress factors do not rebuild to 1e-12 (the three identities above, each up to a phase; checked on the host).
 */
#define SLAM_CX_DRESS 99
int slam_cx_decompose(slam_ctx* ctx, int64_t first, int64_t count, int family, const double* gate, const double* dress, double* x_out,
                      int32_t* cycles, double* loss, double* gap);

/*
 * Closed-form decomposition into one or two gates G of the B class, CAN(1/2, 1/4, 0), on the device, one thread per resident target
 * (csrc/slam_b.hpp; Zhang, Vala, Sastry, Whaley, PRL 93, 020502: two B gates reach every two-qubit unitary).  For the resident targets
 * [first, first + count) (nothing is uploaded, no gate table is needed):
 *   gate    double[32]         G, row-major (re, im)
 *   dress   double[SLAM_B_DRESS]  the host's reduction of G: four 2x2 factors (row-major re, im; in a pair the factor of the qubit of
 *                              the high bit comes first) l1, l0, r1, r0, then c[3], with  G = e^{i .} (l1 (x) l0) CAN(c) (r1 (x) r0),
 *                              c the KAK coordinates of G (within 4e-8 of (1/2, 1/4, 0) once folded to c1 <= 1/2)
 *   x_out   double[count][24]  the 6 (k + 1) template angles in the index order of slam_eval_unitary in the front of the row, zeros
 *                              behind: template(x, [G] * k) = e^{i phi} T
 *   cycles  int32[count]       k: on the coordinates rounded to 8 digits and folded to c1 <= 1/2 (span_rules.minimal_span, tolerance
 *                              2e-8) 1 in G's own class, else 2; a local target gets two gates
 *   loss    double[count]      1 - |Tr(T^+ template(x_out))| / 4, from a forward pass of the written row
 *   gap     double[count]      max-norm distance (units of pi) that remains between the chamber points when the interior circuit is
 *                              aligned with the target, as slam_complete_locals' gap_out: rounding only for two gates
 * Any output pointer may be NULL.  SLAM_ERR_INVALID for a NULL context, a window outside the resident batch, a gate outside the class
 * and a gate that the dress factors do not rebuild to 1e-12 (up to a phase; checked on the host before anything is written).
 */
#define SLAM_B_DRESS 35
int slam_b_decompose(slam_ctx* ctx, int64_t first, int64_t count, const double* gate, const double* dress, double* x_out, int32_t* cycles,
                     double* loss, double* gap);

/*
 * Fidelity-aware approximate decomposition into gates G of the CNOT class (family 0), the iSWAP class (family 1) or the B class
 * (family 2) on the device, one thread per resident target (csrc/slam_approx.hpp; the basis_fidelity half of qiskit's
 * TwoQubitBasisDecomposer, which the reference's pass calls at src/slam/utils/transpiler_pass/weyl_decompose.py:475-480).  For the
 * target's coordinates folded to c1 <= 1/2, (a, b, c) = pi/2 (c1, c2, c3), and G's class (1/2, beta, 0), beta' = pi beta / 2, the best
 * circuit of k gates reaches |Tr(T^+ W)| = 4 t_k:
 *     t_0 = |cos a cos b cos c + i sin a sin b sin c|,
 *     t_1 = |cos(pi/4 - a) cos(beta' - b) cos c + i sin(pi/4 - a) sin(beta' - b) sin c|,
 *     t_2 = |cos c| (families 0, 1), 1 (family 2),     t_3 = 1 (families 0, 1; family 2 has no k = 3),
 * with the loss L_k = 1 - t_k, the average gate fidelity F_k = (4 + 16 t_k^2) / 20 and the expected fidelity E_k = F_k f^k for the
 * fidelity f of one basis gate.  The k with the largest E_k is chosen, compared in the order 0, 1, 2, 3 with strict >: ties go to fewer
 * gates; with f = 1 that is the fewest gates that equal the target, 0 for a local one.
 *   gate, dress     as slam_cx_decompose takes them (families 0, 1; double[SLAM_CX_DRESS]) or slam_b_decompose (family 2;
 *                   double[SLAM_B_DRESS]), checked in the same way
 *   basis_fidelity  f, in (0, 1]
 *   force_cycles    -1: select; 0..3 (0..2 for family 2): that size for every target
 *   x_out   double[count][24]  the 6 (k + 1) template angles in the front of the row, zeros behind; a row of no gate holds one layer
 *   cycles  int32[count]       k
 *   loss    double[count]      1 - |Tr(T^+ template(x_out))| / 4, from a forward pass of the written row
 *   predicted double[count]    L_k of the chosen k, from the formulas above on the unrounded coordinates
 *   gap     double[count]      max-norm distance (units of pi) between the chamber points of the target and of the circuit after the
 *                              alignment: the distance to the nearest point that k gates reach
 * Any output pointer may be NULL.  Arguments are checked before the context.  SLAM_ERR_INVALID for an unknown family, a gate that
 * the dress factors do not rebuild, a basis_fidelity outside (0, 1] or not finite, force_cycles out of range, a NULL context and a
 * window outside the resident batch.
 */
int slam_approx_decompose(slam_ctx* ctx, int64_t first, int64_t count, int family, const double* gate, const double* dress,
                          double basis_fidelity, int force_cycles, double* x_out, int32_t* cycles, double* loss, double* predicted,
                          double* gap);

/*
 * The same selection for n_fid basis fidelities at once, counted: one launch over the resident targets [first, first + count).
 *   fidelities  double[n_fid]      each in (0, 1]; n_fid in 1..64
 *   counts_out  int64[n_fid][4]    targets per chosen size k = 0..3
 *   fidsum_out  int64[n_fid]       the sum over the targets of llrint(E_k 2^32) for the chosen k: fixed point, so counts and sums do not
 *                                  depend on the order of addition
 * Any output pointer may be NULL.  SLAM_ERR_INVALID for an unknown family, n_fid or a fidelity out of range, a NULL context and a
 * window outside the resident batch.
 */
int slam_approx_counts(slam_ctx* ctx, int64_t first, int64_t count, int family, int32_t n_fid, const double* fidelities,
                       int64_t* counts_out, int64_t* fidsum_out);

/*
 * The same decomposition into gates G of ANY supercontrolled class CAN(1/2, beta, 0), 0 <= beta <= 1/2 (csrc/slam_sc.hpp): the line of
 * the Weyl chamber through the CNOT (beta = 0), the B (1/4) and the iSWAP class (1/2), every full-strength conversion-gain gate
 * included.  Three such gates reach every target (the construction of qiskit's TwoQubitBasisDecomposer); the t_k, F_k, E_k and the
 * selection are those of slam_approx_decompose with the gate's own beta, t_2 = |cos c| and t_3 = 1 for every beta.  For
 * 0 < beta < 1/2 two gates reach more than the plane c3 = 0, but this two-gate formula is exact on the plane only: a target off it
 * gets three gates at f = 1 (at beta = 1/4 slam_b_decompose returns two for every target).
 *   gate    double[32]            G, row-major (re, im)
 *   dress   double[SLAM_SC_DRESS] the host's reduction of G as slam_b_decompose takes it: l1, l0, r1, r0, then c[3], with
 *                                 G = e^{i .} (l1 (x) l0) CAN(c) (r1 (x) r0), c within 4e-8 of (1/2, beta, 0) once folded to c1 <= 1/2.
 *                                 The constant matrices of the construction depend on beta alone; the library forms them itself and
 *                                 folds l and r into them
 *   basis_fidelity, force_cycles (-1, 0..3), x_out, cycles, loss, predicted, gap   as slam_approx_decompose
 * Any output pointer may be NULL.  Arguments are checked before the context.  SLAM_ERR_INVALID for a gate off the line, a gate that
 * the dress factors do not rebuild to 1e-12, a basis_fidelity outside (0, 1] or not finite, force_cycles out of range, a NULL
 * context and a window outside the resident batch; nothing is written then.
 */
#define SLAM_SC_DRESS 35
int slam_sc_decompose(slam_ctx* ctx, int64_t first, int64_t count, const double* gate, const double* dress, double basis_fidelity,
                      int force_cycles, double* x_out, int32_t* cycles, double* loss, double* predicted, double* gap);

/* The sweep of slam_approx_counts for such a gate: gate and dress as slam_sc_decompose, the rest as slam_approx_counts. */
int slam_sc_counts(slam_ctx* ctx, int64_t first, int64_t count, const double* gate, const double* dress, int32_t n_fid,
                   const double* fidelities, int64_t* counts_out, int64_t* fidsum_out);

/*
 * The same decomposition into gates S = sqrt(iSWAP) = RiSwapGate(1/2), the gate of slam_sqiswap_decompose, which is not supercontrolled
 * (csrc/slam_sqapprox.hpp): per target the circuit of 0, 1, 2 or 3 S with the highest expected fidelity.  Coordinates in units of pi,
 * folded to (x, y, z) = (c1, c2, c3), or (1 - c1, c2, -c3) where c1 > 1/2; w = |z|, s = sign(z);
 * ov(d) = |Tr CAN(d)| / 4 = sqrt((cos d1' cos d2' cos d3')^2 + (sin d1' sin d2' sin d3')^2), d' = pi d / 2.  The best circuit of k
 * gates reaches |Tr(T^+ W)| = 4 t_k:
 *     t_0 = ov(x, y, z),     t_1 = ov(1/4 - x, 1/4 - y, z),     t_3 = 1,
 *     t_2 = 1 inside the region w <= x - y that two S reach (tested as slam_sqiswap_decompose tests its size: on coordinates rounded to
 *           8 digits, with 2e-8 of tolerance); outside it t_2 = ov(p - (x, y, z)) for the nearest point p of the region: with
 *           u = (w - x + y) / 3, p = (x + u, y - u, s (w - u)), or, where x + u > 1/2, p = (1/2, y - r / 2, s (w - r / 2)) with
 *           r = y + w - 1/2 (the ridge of the region at the fold c1 = 1/2).
 * L_k, F_k, E_k and the selection are those of slam_approx_decompose.  With f = 1: no gate for a local target, one for a target of S's
 * class, otherwise the size of slam_sqiswap_decompose.  Three gates are built as slam_sqiswap_decompose builds them.
 *   basis_fidelity, force_cycles (-1, 0..3), x_out, cycles, loss, predicted, gap   as slam_approx_decompose (gap for three gates: the
 *   gap of slam_sqiswap_decompose)
 * Any output pointer may be NULL.  Arguments are checked before the context.  SLAM_ERR_INVALID for a basis_fidelity outside (0, 1] or
 * not finite, force_cycles out of range, a NULL context and a window outside the resident batch; nothing is written then.
 */
int slam_sqiswap_approx_decompose(slam_ctx* ctx, int64_t first, int64_t count, double basis_fidelity, int force_cycles, double* x_out,
                                  int32_t* cycles, double* loss, double* predicted, double* gap);

/* The sweep of slam_approx_counts for sqrt(iSWAP): the selection of slam_sqiswap_approx_decompose, the rest as slam_approx_counts. */
int slam_sqiswap_approx_counts(slam_ctx* ctx, int64_t first, int64_t count, int32_t n_fid, const double* fidelities, int64_t* counts_out,
                               int64_t* fidsum_out);

/*
 * Span predictor on the device: for every resident target of [first, first + count) the smallest number k of leading gates of a
 * template whose coverage set contains the target -- the lookup CircuitTemplate.get_spanning_range makes with use_polytopes=True
 * (src/slam/basis.py:95-100 -> monodromy_range_from_target, src/slam/utils/polytopes/polytope_wrap.py:39-94).  The coverage sets
 * come from the caller as half-spaces in the target's alcove coordinates (slam_decomposition_amd/coverage.py computes them from the
 * gates' Weyl coordinates):
 *   point   double[4]            alcove point of the first gate (k = 1: the target must be that class)
 *   bounds  double[k_max][14]    row k - 1 (k >= 2; row 0 unused): bounds[p] <= sum of the target's alcove coordinates over the
 *                                p-th subset ({4},{3},{2},{1},{4,3},{4,2},{4,1},{3,2},{3,1},{2,1},{4,3,2},{4,3,1},{4,2,1},{3,2,1} of the
 *                                decreasing coordinates a_1..a_4); -inf = no constraint
 *   tol                          widens the regions (units of pi)
 * spans_out: int32[count]: 0 = local target, 1 .. k_max, k_max + 1 = out of reach of the whole template.  k_max <= 5.
 */
int slam_predict_spans(slam_ctx* ctx, int64_t first, int64_t count, int k_max, const double* point, const double* bounds, double tol,
                       int32_t* spans_out);

/*
 * Coverage lookup on the device: for every resident target of [first, first + count) the first entry of a cost-ordered coverage set
 * whose region contains the target -- the lookup MixedOrderBasisCircuitTemplate makes (src/slam/basis.py:321-326 ->
 * monodromy_range_from_target, src/slam/utils/polytopes/polytope_wrap.py:39-94) for TemplateOptimizer.cost_target_U /
 * cost_from_distribution (src/slam/optimizer.py:156-178).  No optimisation.  Several coverage sets ("tables") are looked up in one
 * call; table t holds entries [table_offsets[t], table_offsets[t + 1]) of one concatenated entry array of E = table_offsets[n_tables]
 * rows, in cost order:
 *   table_offsets  int32[n_tables + 1]  table_offsets[0] = 0, non-decreasing
 *   kinds          int32[E]             0: one gate (the target must be in its class); 1: a circuit of two or more gates
 *   points         double[E][4]         kind 0: the gate's alcove point (|a_j - point_j| <= max(tol, 0) + 1e-12)
 *   bounds         double[E][14]        kind 1: bounds[p] - tol <= sum of the target's alcove coordinates over the p-th subset (the
 *                                       order of slam_predict_spans); -inf = no constraint (all -inf: every target)
 *   tol                                 widens the regions (units of pi)
 * counts_out  int64[E + 2 n_tables]: per table, n_entries + 2 counts -- targets whose first containing entry is entry e (e = 0 ..
 *             n_entries - 1), then local targets, then targets no entry contains.
 * entry_out   int32[n_tables][count] or NULL: per table and target, the same bin index (n_entries = local, n_entries + 1 = none).
 * Integer counts: the result does not depend on the order in which the device adds them up.
 */
int slam_coverage_lookup(slam_ctx* ctx, int64_t first, int64_t count, int32_t n_tables, const int32_t* table_offsets, const int32_t* kinds,
                         const double* points, const double* bounds, double tol, int64_t* counts_out, int32_t* entry_out);

/*
 * Family-extended lookup on the device (recursive_sibling_check, src/slam/utils/gates/family_extend.py:17-117, for every resident
 * target of [first, first + count)): a gate family is a base pulse (member 0) and the same pulse run 2^a 3^b times as long.  Member m
 * has the rows [table_offsets[m], table_offsets[m + 1]) of one concatenated table laid out as for slam_coverage_lookup, row j of a
 * member = j + 1 applications of it, at the cost (j + 2) cost_1q + (j + 1) durations[m].
 *   policy 0  the reference's walk: k = the first row of the member that contains the target; stop at k = 1; else go on to
 *             child_even[m] (k even) or child_odd[m] (k odd), stop if that is -1 or does not contain the target; unwinding, a level
 *             keeps its child's result only where that is strictly cheaper;
 *   policy 1  the cheapest over ALL members that contain the target (ties: the smaller member index).
 * A local target takes no gate (cost 0); a target that member 0 does not contain is unreachable, under both policies.
 *   n_members                1 .. SLAM_FAMILY_MAX_MEMBERS, every member with at least one row, E + E_0 + 4 <= 8192
 *   child_even, child_odd    int32[n_members]: -1, or an index GREATER than the member's own
 *   durations                double[n_members], finite
 * counts_out       int64[E + 2]: targets that ended on each row, then local targets, then unreachable ones.
 * base_counts_out  int64[E_0 + 2], E_0 = table_offsets[1]: the same for member 0 alone (no family), from the same pass.
 * member_out, gates_out  int32[count] or NULL: member index and number of gates per target; -1 / 0 local, -1 / -1 unreachable.
 * Integer counts: the result does not depend on the order in which the device adds them up.
 */
#define SLAM_FAMILY_MAX_MEMBERS 32
int slam_family_lookup(slam_ctx* ctx, int64_t first, int64_t count, int32_t n_members, const int32_t* table_offsets, const int32_t* kinds,
                       const double* points, const double* bounds, const int32_t* child_even, const int32_t* child_odd,
                       const double* durations, double cost_1q, double tol, int32_t policy, int64_t* counts_out,
                       int64_t* base_counts_out, int32_t* member_out, int32_t* gates_out);

/*
 * Candidate basis-gate scores on the device (collect_data, src/slam/utils/gates/bare_candidates.py:75-126, for a whole grid of
 * candidates at once): for every candidate gate g and every resident target t of [first, first + count) the smallest k in 1 .. k_cap
 * such that k applications of g, with free local gates in between, reach t -- coverage.contains(t, [g] * k, tol): the alcove-point match
 * of slam_coverage_lookup kind 0 for k = 1, the 14 half-spaces of kind 1 for k >= 2; either alcove point of the target's class may
 * match.  The device derives every row from the candidate's three coordinates (the max-plus recurrence of coverage._region with the
 * degree folded into the weight, csrc/slam_candidates.hpp): no table comes from the caller.
 *   cand_coords  double[n_candidates][3]  Weyl coordinates in units of pi (weyl.c1c2c3); 1 <= n_candidates <= SLAM_CANDIDATE_MAX_GATES
 *   k_cap        1 .. SLAM_CANDIDATE_MAX_K
 *   tol          widens the regions (units of pi), as in slam_coverage_lookup
 *   group_of     int32[count] or NULL: the group (0 .. n_groups - 1) of every target of the window; NULL = one group (n_groups = 1)
 * counts_out    int64[n_groups][n_candidates][k_cap + 2]: bin k - 1 = targets first reached at k; bin k_cap = local targets (no gate);
 *               bin k_cap + 1 = targets not reached within k_cap.  A local candidate reaches no non-local target.
 * first_k_out   int32[n_candidates][count] or NULL: k per (candidate, target); 0 = local target, k_cap + 1 = not reached.
 * kernel_ms_out double* or NULL: device time of the call's two kernels (events on the context's stream).
 * Integer counts: the result does not depend on the launch geometry, the window or the order in which the device adds them up.
 */
#define SLAM_CANDIDATE_MAX_K 64
#define SLAM_CANDIDATE_MAX_GATES 65536
int slam_candidate_scores(slam_ctx* ctx, int64_t first, int64_t count, int32_t n_candidates, const double* cand_coords, int32_t k_cap,
                          double tol, const int32_t* group_of, int32_t n_groups, int64_t* counts_out, int32_t* first_k_out,
                          double* kernel_ms_out);

/*
 * Parallel-drive coverage (the sampling half of src/slam/utils/gates/parallel_drive_volume.py:176-256; csrc/slam_pd.hpp).
 *
 * slam_pd_sample: n_samples random templates of k ConversionGainSmushGate(pc, pg, gc, gg, gx[0:N], gy[0:N], t), N = n_slices, with a
 * U3 (x) U3 layer between consecutive gates and none outside (CircuitTemplateV2(no_exterior_1q=1, vz_only=0,
 * param_vec_expand=[2, N, N])).  Every parameter is uniform in (-bound, bound), drawn on the device from Philox4x32-10 keyed
 * (seed, sample index, k); sample i has index first_index + i, or indices[i] when indices is not NULL (replay of chosen samples).
 * Each slice is exp(-i (t / N) H) of the full Hermitian H (free phases).  The Weyl coordinates of every product (8 digits with
 * ndigits = 8, unrounded with ndigits < 0), folded to c1 <= 1/2, stay resident for slam_pd_extremes / slam_pd_filter.  Optional
 * host outputs (NULL = not wanted): coords_out double[n][3]; params_out double[n][P], P = 6 (k - 1) + k (2 + 2N), in the template's
 * index order (layer angles, then per gate pc, pg, gx[0..N), gy[0..N)); unitaries_out double[n][4][4][2].
 * k in 1..SLAM_PD_MAX_SPAN and n_slices in 1..SLAM_PD_MAX_SLICES (else SLAM_ERR_UNSUPPORTED); t > 0, bound > 0, n_samples >= 1.
 *
 * slam_pd_extremes: for each of n_dirs directions (double[n_dirs][3]) the resident sample with the largest dot product (values
 * compared in float precision, ties to the lower index): index_out int64[n_dirs], coords_out double[n_dirs][3].
 *
 * slam_pd_filter: the resident samples that are NOT strictly inside (by more than eps) every facet n . c <= b of facets
 * double[n_facets][4] = (n, b) -- with the facets of the hull of some samples, exactly those that can be vertices of the hull of all
 * of them.  *n_out = how many; the first min(*n_out, capacity) go to index_out int64[] / coords_out double[][3], in no fixed order.
 */
#define SLAM_PD_MAX_SPAN 8
#define SLAM_PD_MAX_SLICES 16
#define SLAM_PD_MAX_DIRS 1024
#define SLAM_PD_MAX_FACETS (1 << 20)
int slam_pd_sample(slam_ctx* ctx, double gc, double gg, double t, int32_t n_slices, int32_t k, double bound, uint64_t seed,
                   int64_t first_index, int64_t n_samples, const int64_t* indices, int ndigits, double* coords_out, double* params_out,
                   double* unitaries_out);
int slam_pd_extremes(slam_ctx* ctx, const double* directions, int32_t n_dirs, int64_t* index_out, double* coords_out);
int slam_pd_filter(slam_ctx* ctx, const double* facets, int32_t n_facets, double eps, int64_t capacity, int64_t* n_out, int64_t* index_out,
                   double* coords_out);

/*
 * Region lookup on the device: the resident targets [first, first + count) against n_regions regions (<= SLAM_REGION_MAX), each a
 * union of polytopes [region_offsets[r], region_offsets[r + 1]).  Polytope p has kinds[p]:
 *   0  facets [facet_offsets[p], facet_offsets[p + 1]) of facets double[][4] = (n, b): inside iff n . c <= b + tol for all of them,
 *      c = the target's Weyl coordinates (8 digits, c3 >= 0)
 *   1  a coverage region of two or more gates: aux[p][0..14) = bounds as in slam_coverage_lookup kind 1
 *   2  one gate's class: aux[p][0..4) = its alcove point as in slam_coverage_lookup kind 0
 * aux: double[P][14] (may be NULL when every kind is 0); facet_offsets int32[P + 1] (P = region_offsets[n_regions]).
 * counts_out int64[2 n_regions + 1]: targets inside region r (r = 0 .. n_regions - 1), then targets whose FIRST containing region is r,
 * then targets in none.  Integer counts: the result does not depend on the order in which the device adds them up.
 */
#define SLAM_REGION_MAX 256
int slam_region_lookup(slam_ctx* ctx, int64_t first, int64_t count, int32_t n_regions, const int32_t* region_offsets, const int32_t* kinds,
                       const int32_t* facet_offsets, const double* facets, const double* aux, double tol, int64_t* counts_out);

/*
 * Upload the table of 2Q basis-gate matrices (CircuitTemplate(base_gates=...),
 * src/slam/basis.py:52-69; matrices from src/slam/utils/gates/custom_gates.py).
 * gates: double[n_gates][4][4][2].
 */
int slam_set_gates(slam_ctx* ctx, const double* gates, int32_t n_gates);

/*
 * Fused forward chain + BasicCost + analytic gradient for M independent items.
 * Replaces objective_func (src/slam/optimizer.py:191-214) = CircuitTemplate.eval
 * (src/slam/basis.py:102-104) + BasicCost.unitary_fidelity
 * (src/slam/cost_function.py:140-145), and SciPy's finite-difference gradient
 * (src/slam/optimizer.py:270-278, no jac) with the analytic one.
 *   k          span (number of 2Q gates), 1..SLAM_MAX_SPAN_EVAL
 *   gate_seq   int32[k]: index into the gate table for G_1..G_k
 *   x          double[M][6(k+1)]
 *   target_of  int32[M]: target index of each item
 *   loss       double[M]           (out)
 *   grad       double[M][6(k+1)]   (out, may be NULL)
 */
int slam_eval_loss_grad(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x,
                        const int32_t* target_of, int64_t M, double* loss, double* grad);

/*
 * CircuitTemplate.eval (src/slam/basis.py:102-104) for M parameter vectors: the 4x4 template
 * unitary W(x) = K_k G_k ... G_1 K_0, as qiskit's Operator(circuit).data returns it.
 *   unitary    double[M][4][4][2]  (out)
 *   loss       double[M]           (out, may be NULL) BasicCost against target_of[m]
 */
int slam_eval_unitary(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x,
                      const int32_t* target_of, int64_t M, double* unitary, double* loss);

/*
 * One span stage of TemplateOptimizer._run (src/slam/optimizer.py:233-303) for a
 * batch: for every active target run `restarts` independent quasi-Newton (BFGS)
 * minimisations from different seeds and return the best.
 * Replaces the `for r_i in range(training_restarts): opt.minimize(...)` loop
 * (optimizer.py:253-295) and parameter_guess (basis.py:106-111).
 *   active        int32[n_active] target indices (NULL = all targets 0..n_targets-1)
 *   x0            optional double[n_active][R][n] explicit seeds (NULL = Philox from params->seed,
 *                 counter = (pair index, restart, target index, k))
 *   best_loss     double[n_active]      (out)
 *   best_x        double[n_active][n]   (out)
 *   best_restart  int32[n_active]       (out, may be NULL)
 *   item_loss     double[n_active][R]   (out, may be NULL)  per-restart final loss
 *   item_iters    int32[n_active][R]    (out, may be NULL)
 *   item_status   int32[n_active][R]    (out, may be NULL)  SLAM_ST_*
 *   item_evals    int32[n_active][R]    (out, may be NULL)  loss+grad evaluations used
 */
int slam_minimize_stage(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active,
                        int64_t n_active, const double* x0, const slam_opt_params* params,
                        double* best_loss, double* best_x, int32_t* best_restart,
                        double* item_loss, int32_t* item_iters, int32_t* item_status,
                        int32_t* item_evals);

/*
 * The whole span loop of TemplateOptimizer._run for the resident batch
 * (src/slam/optimizer.py:233-303): spans k = k_min..k_max; after each span the targets
 * whose best loss is < success_threshold leave the batch (optimizer.py:301-303), the
 * rest continue with the next span.  Compaction stays on the device; only the final
 * per-target results return.
 *   gate_seqs   int32[(k_max)(k_max+1)/2 ...] concatenated sequences for k = k_min..k_max
 *               (k_min entries, then k_min+1, ...)
 *   best_loss   double[n_targets]            (out)
 *   best_x      double[n_targets][6(k_max+1)] (out; first 6(best_cycles+1) entries valid)
 *   best_cycles int32[n_targets]             (out) span of the best result (optimizer.py:284)
 */
int slam_decompose(slam_ctx* ctx, int k_min, int k_max, const int32_t* gate_seqs,
                   const slam_opt_params* params, double success_threshold, double* best_loss,
                   double* best_x, int32_t* best_cycles);

/* Same as slam_decompose but leaves the results on the device (bench timing without D2H).
 * Fetch them afterwards with slam_fetch_results. */
int slam_decompose_resident(slam_ctx* ctx, int k_min, int k_max, const int32_t* gate_seqs,
                            const slam_opt_params* params, double success_threshold);
int slam_fetch_results(slam_ctx* ctx, int k_max, double* best_loss, double* best_x,
                       int32_t* best_cycles);

/* The same span loop restricted to the window [first, first + count) of the resident targets
 * (results of other targets are left untouched): lets a caller keep many batches resident and
 * process them one after the other, or overlap batches from several host threads' contexts. */
int slam_decompose_range(slam_ctx* ctx, int64_t first, int64_t count, int k_min, int k_max,
                         const int32_t* gate_seqs, const slam_opt_params* params,
                         double success_threshold);
/* slam_decompose_range followed by slam_fetch_results_range(ctx, k_max, first, count, ...) with one host wait
 * instead of two: the result copies are enqueued behind the last stage. */
int slam_decompose_range_fetch(slam_ctx* ctx, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs,
                               const slam_opt_params* params, double success_threshold, double* best_loss, double* best_x,
                               int32_t* best_cycles);

/* The span loops of SEVERAL contexts in one chain of kernels (round 4): n_ctx contexts on one device, each holding the target
 * window [first, first + count) and ITS OWN gate table (slam_set_gates) -- the bases of a basis-gate sweep
 * (src/slam/utils/gates/bare_candidates.py:47-69 builds such a family; the reference then runs one TemplateOptimizer per gate).
 * Per span ONE optimizer launch serves all of them -- a wavefront works on one context's queue at a time, so the gates stay scalar
 * operands -- and one bookkeeping launch.  Every context ends with exactly the resident results its own slam_decompose_range
 * call would have left (needs SLAM_FLAG_EARLY_EXIT | SLAM_FLAG_ORDERED: results independent of scheduling); fetch them per
 * context with slam_fetch_results_range.  Spans 1..3; the work is enqueued on ctxs[0]'s stream, whose statistics get the kernel
 * times (evaluation counts go to each context's own statistics).  The contexts must be idle and distinct. */
int slam_decompose_multi(slam_ctx** ctxs, int32_t n_ctx, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs,
                         const slam_opt_params* params, double success_threshold);

/* The same for an explicit list of resident-target indices (e.g. the targets a span predictor assigns to one
 * template size: CircuitTemplate.get_spanning_range with use_polytopes, src/slam/basis.py:95-100).  Results land
 * in the per-target resident arrays like those of slam_decompose_range; fetch them with
 * slam_fetch_results_range(ctx, k_layout, ...): rows of best_x are 6 (k_layout + 1) wide, so that lists with
 * different k_max can share one resident result set (k_layout = 0 means k_max). */
int slam_decompose_list(slam_ctx* ctx, const int32_t* targets, int64_t count, int k_min, int k_max, int k_layout,
                        const int32_t* gate_seqs, const slam_opt_params* params, double success_threshold);
int slam_fetch_results_range(slam_ctx* ctx, int k_max, int64_t first, int64_t count,
                             double* best_loss, double* best_x, int32_t* best_cycles);

/*
 * CircuitTemplate(use_polytopes=True) for the resident targets [first, first + count) in ONE chain of kernels (round 5): the template
 * size every target needs is looked up on the device (the half-spaces of slam_predict_spans: `point`, `bounds[k_max][14]`, `tol`), the
 * targets are sorted into per-size lists there, and one span loop runs in which the targets of size k join at stage k -- what
 * get_spanning_range + _run do per target in the reference (src/slam/basis.py:95-100 -> utils/polytopes/polytope_wrap.py:39-94,
 * src/slam/optimizer.py:233-303), without the host's per-size index lists and one slam_decompose_list call per size.
 *   carry = 0  exact regions: a target runs at its own size only (the reference's range(k, k + 1));
 *   carry = 1  a target that misses success_threshold at its size goes on to the next one (lower bounds, widened regions).
 * gate_seqs: the sequences of spans 1 .. k_max, concatenated.  Results stay resident (rows 6 (k_max + 1) wide: fetch with
 * slam_fetch_results_range(ctx, k_max, ...)); a local target (size 0) gets (loss 0, cycles 0), a target out of the template's reach
 * (+inf, -1); their numbers come back in n_local / n_unreachable (either may be NULL).
 */
int slam_decompose_predicted(slam_ctx* ctx, int64_t first, int64_t count, int k_max, const double* point, const double* bounds, double tol,
                             int carry, const int32_t* gate_seqs, const slam_opt_params* params, double success_threshold,
                             int64_t* n_local, int64_t* n_unreachable);

/*
 * Running best loss of resident targets [first, first + count) after every span the span loop ran for them:
 * out[t][k - 1] = best loss after span k, NaN where the target did not run span k (solved earlier, or k outside the
 * call's range) -- the value of the reference's "Cycle (k =...), Best Loss=..." log line (src/slam/optimizer.py:297).
 * out: double[count][SLAM_MAX_SPAN_EVAL].
 */
int slam_fetch_span_losses(slam_ctx* ctx, int64_t first, int64_t count, double* out);

/*
 * slam_minimize_stage with the per-iteration trajectories the reference collects through SciPy's callback when
 * use_callback=True (callbackF, src/slam/optimizer.py:217-224: loss and point after every BFGS iteration):
 *   trace_loss  double[n_active][R][trace_cap]      loss after accepted step number it at [it - 1], NaN beyond item_iters
 *   trace_x     double[n_active][R][trace_cap][n]   parameters at the same point (feed slam_eval_c1c2c3 for the
 *                                                   coordinate trajectory of optimizer.py:223-224)
 *   exit_loss   with SLAM_FLAG_EARLY_EXIT | SLAM_FLAG_ORDERED: a restart that ends below it stops the restarts of
 *               HIGHER index only, so every restart up to the first successful one runs to its end -- what the
 *               reference's sequential loop records (the span loop's success threshold, optimizer.py:287)
 * Meant for a few targets at a time (the trace must fit 4 GiB).  Spans 1..SLAM_MAX_SPAN_MINIMIZE (both kernel families, round 5).
 */
int slam_minimize_stage_trace(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active,
                              const double* x0, const slam_opt_params* params, double exit_loss, int32_t trace_cap,
                              double* best_loss, double* best_x, int32_t* best_restart, double* item_loss,
                              int32_t* item_iters, int32_t* item_status, double* trace_loss, double* trace_x);

/*
 * Objective used by every later evaluation / minimisation of this context
 * (UnitaryCostFunction subclasses, src/slam/cost_function.py):
 *   SLAM_COST_BASIC   BasicCost   1 - |Tr(T^+ U)| / d                       (cost_function.py:140-145), default
 *   SLAM_COST_SQUARE  SquareCost  1 - (|Tr(T^+ U)|^2 + d) / (d (d + 1))     (cost_function.py:169-173)
 *   SLAM_COST_MAKHLIN MakhlinFunctionalCost  sum_i (g_i(U) - g_i(T))^2       (cost_function.py:219-221, weylchamber J_T_LI)
 *                     with g = (Re G1, Im G1, Re G2) the Makhlin local invariants: the distance up to single-qubit gates.  Unrounded
 *                     (the reference's invariants are rounded to 8 digits).  Honoured by slam_eval_loss_grad, slam_eval_unitary,
 *                     slam_minimize_stage(_trace), slam_decompose, slam_decompose_range(_fetch), slam_decompose_list /
 *                     _resident and slam_decompose_predicted -- always through the per-span launches (as SLAM_FLAG_STAGED |
 *                     SLAM_FLAG_NO_OVERLAP), whatever the flags say.  slam_decompose_multi and the slam_v2_* family return
 *                     SLAM_ERR_UNSUPPORTED under it.
 * Anything else fails like the reference's objective_func: "Unrecognized Cost Function" (optimizer.py:211).
 */
#define SLAM_COST_BASIC 0
#define SLAM_COST_SQUARE 1
#define SLAM_COST_MAKHLIN 2
int slam_set_cost(slam_ctx* ctx, int cost);

/* Block until all work queued on the context's stream has finished. */
int slam_synchronize(slam_ctx* ctx);

/* Page-locked host memory for result arrays (round 5).  The fetch entry points (slam_decompose_range_fetch, slam_fetch_results_range,
 * slam_v2_decompose_range ...) copy straight into the caller's arrays; when those are ordinary pageable memory the runtime pins and
 * unpins them around every copy, and FREEING such arrays later (munmap / heap trimming of tens of MB) was measured to stall every queue
 * of the process for 13-18 ms at the start of the next call (profiles/r5_api_timeline.txt).  Arrays from slam_host_alloc are visible to
 * every device, are copied into by DMA without staging, and are meant to be recycled by the caller (the Python binding keeps a pool).
 * Use them for ONE blocking call at a time (18.2 -> 16.9 ms for 65 536 x 32 sqrt(iSWAP) through the Python API); with several calls in
 * flight the device-side copy waits for wave slots behind the other calls' kernels and pageable arrays are faster (14.4 vs 14.9 ms per step).
 * Replaces nothing in the reference (its results are Python lists built on the host, src/slam/optimizer.py:113-119). */
int slam_host_alloc(size_t bytes, void** ptr);
int slam_host_free(void* ptr);

/* Accumulated kernel statistics since the last reset. */
int slam_get_stats(slam_ctx* ctx, slam_stats* out);
int slam_reset_stats(slam_ctx* ctx);

/* Device pointer + byte size of the resident per-target best-loss array
 * (double[n_targets]); used by the multi-GPU merge to hand the buffer to RCCL
 * without a host round trip. */
int slam_best_loss_device_ptr(slam_ctx* ctx, void** ptr, int64_t* n);

/*
 * Device check of the quasi-Newton metric's rank-2 update H += s w^T + v s^T (csrc/slam_device.hpp: h_update), one quad per item as
 * in the optimizer kernels.  The update is applied to the caller's blocks once through the form the optimizer kernels run (the
 * 4x4x1 fp32 MFMA where an instantiation has it) and once through the v_pk_fma_f32 form, which this kernel keeps as the reference;
 * the two are expected to agree bit for bit (tests/test_gpu_metric_mfma.py).  na = slots per lane: 3, 5, 6 (spans 1, 2, 3).
 *   h                     float[n_items][na (na + 1) / 2][4][4]  upper blocks, block (a, b), a <= b, at b (b + 1) / 2 + a;
 *                                                                 element [q][e] = H[4a + q][4b + e]
 *   s, w, v               float[n_items][4 na]                   component 4a + q
 *   h_shipped, h_vector   like h (out)
 */
int slam_metric_update_check(slam_ctx* ctx, int na, const float* h, const float* s, const float* w, const float* v, int64_t n_items,
                             float* h_shipped, float* h_vector);

/* HIP device ordinal the context was created on (slam_comm_merge_add checks it against its communicator's). */
int slam_ctx_device(slam_ctx* ctx, int* device);

/*
 * Templates whose 2Q gates carry their own optimisable parameters -- CircuitTemplateV2 (src/slam/basisv2.py:27-299):
 * base_gates are gate classes / lambdas, every gate instance of the circuit gets its own "Q" parameters next to the "P"
 * parameters of the U gates, optionally box-bounded (add_bound, basisv2.py:174-190; the reference then switches SciPy to
 * L-BFGS-B, src/slam/optimizer.py:255-268).  Supported gate family: conversion-gain gates
 *     G(a, phi_c, b, phi_g) = exp(-i t H),  H = gc (e^{i phi_c} A B^+ + h.c.) + gg (e^{i phi_g} A B + h.c.),  a = gc t,  b = gg t
 * (ConversionGainGate, custom_gates.py:163-212; hamiltonian.py:84-111), which contains RiSwapGate(alpha) =
 * G(-pi alpha / 2, 0, 0, 0) (custom_gates.py:534-606).  A slam_v2_gate says how the four raw angles, in the order
 * (a, phi_c, b, phi_g), follow from the gate's n_params parameters q: raw[r] = scale[r] * q[sel[r]] + offset[r]
 * (sel[r] = -1: the constant offset[r]).  n_params is 1, 2 or 4 and the same for every gate of a template.
 *
 * Parameter vectors are in index order: P0 .. P{6(k+1)-1} as for fixed-gate templates, then the parameters of gate 1,
 * of gate 2, ...: n = 6 (k + 1) + n_params k.  Spans 1..3 for every n_params; span 4 for n_params <= 2 and span 5
 * (the reference's default maximum_span_guess, basisv2.py:35) for n_params = 1 -- as long as the packed inverse Hessian of
 * the n parameters fits one wavefront's registers (n <= 41); beyond that SLAM_ERR_UNSUPPORTED.
 *
 *   slam_v2_set_gates        the table of parametrised base gates (host side only; replaces nothing resident)
 *   slam_v2_eval_loss_grad   loss, gradient with respect to ALL n parameters (analytic, incl. the gate parameters) and
 *                            (optional) the template unitary of M parameter vectors -- objective_func
 *                            (optimizer.py:191-214) for a CircuitTemplateV2
 *   slam_v2_minimize_stage   one span stage: per active target `restarts` projected quasi-Newton minimisations
 *                            (BFGS metric, steps projected onto the box [bound_lo, bound_hi]; NULL bounds = none, which
 *                            is plain BFGS as in optimizer.py:255).  Start points: x0, or U[init_lo, init_hi) per
 *                            parameter from the Philox stream of params->seed (parameter_guess, basisv2.py:150-172:
 *                            the bound of a bounded parameter, else (-4 pi, 4 pi)).  The stage result is the
 *                            lowest-index restart below exit_loss, else the lowest loss -- the restart the reference's
 *                            sequential loop ends with (optimizer.py:281-295).  With SLAM_FLAG_EARLY_EXIT in
 *                            params->flags a restart is not started once a LOWER-index restart of its target has
 *                            ended below exit_loss (the loop's break); without it every restart runs to its end.
 *                            Persistent wavefronts over a restart-major queue, as slam_minimize_stage.
 *                            Outputs as in slam_minimize_stage with rows of n parameters.
 *   slam_v2_set_constraint   CircuitTemplateV2.set_constraint (basisv2.py:192-200: circuit_cost(x) <= param_max_cost, handed to
 *                            SciPy's SLSQP by optimizer.py:260-265) for circuit costs that are affine in the parameters over
 *                            the box: sum_i weights[i] x_i <= cost_max for the span-k template (n = its parameter count, index
 *                            order; RiSwapGate.cost() = alpha: weight 1 on every gate parameter).  Every later stage of that
 *                            span minimises the augmented Lagrangian loss + rho / 2 max(0, w.x - cost_max + mu / rho)^2 over the
 *                            box with the same projected quasi-Newton loop and updates the multiplier estimate mu per item
 *                            until w.x <= cost_max and mu (w.x - cost_max) = 0 to 1e-8; returned points are feasible, the
 *                            returned loss is the plain loss.
 *                            weights = NULL or n = 0 removes the constraint of span k (remove_constraint, basisv2.py:202-204);
 *                            slam_v2_set_gates removes all of them.
 */
#define SLAM_V2_MAX_SPAN 5 /* spans 4 and 5 for gates with few parameters: see slam_v2_minimize_stage */
typedef struct slam_v2_gate {
    int32_t n_params;
    int32_t sel[4];
    double scale[4];
    double offset[4];
} slam_v2_gate;
int slam_v2_set_gates(slam_ctx* ctx, const slam_v2_gate* gates, int32_t n_gates);
int slam_v2_set_constraint(slam_ctx* ctx, int k, const double* weights, int n, double cost_max);
int slam_v2_eval_loss_grad(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x, const int32_t* target_of, int64_t M,
                           double* loss, double* grad, double* unitary);
int slam_v2_minimize_stage(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active, const double* x0,
                           const double* init_lo, const double* init_hi, const double* bound_lo, const double* bound_hi,
                           const slam_opt_params* params, double exit_loss, double* best_loss, double* best_x, int32_t* best_restart,
                           double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals);

/* The whole span loop of a CircuitTemplateV2 (TemplateOptimizer._run, src/slam/optimizer.py:233-303, with a V2 template) for the
 * resident targets [first, first + count), enqueued as one chain of kernels like slam_decompose_range: per span k = k_min..k_max the
 * V2 optimizer kernel over the targets still above success_threshold (ordered early exit per params->flags), the reduction over
 * restarts, the merge into the running best and the compaction -- no host round trip between the spans.
 *   gate_seqs                        concatenated gate sequences (k_min entries, then k_min + 1, ...), indices into slam_v2_set_gates' table
 *   init_lo/hi, bound_lo/hi          concatenated per span: n_k = 6 (k + 1) + n_params k entries for k = k_min, then k_min + 1, ...
 *                                    (bound_* may be NULL: no bounds)
 *   best_loss [count], best_cycles [count], best_x [count][n_kmax]: a target solved at span k has the n_k parameters of that
 *   span's layout in the front of its row, zeros behind (any of the three may be NULL). */
int slam_v2_decompose_range(slam_ctx* ctx, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs, const double* init_lo,
                            const double* init_hi, const double* bound_lo, const double* bound_hi, const slam_opt_params* params,
                            double success_threshold, double* best_loss, double* best_x, int32_t* best_cycles);

/* slam_v2_minimize_stage that also records every accepted iteration of every restart (use_callback=True for a
 * CircuitTemplateV2, src/slam/optimizer.py:217-224): trace_loss [M][trace_cap], trace_x [M][trace_cap][n] as
 * slam_minimize_stage_trace; rows no iteration reaches read as NaN. */
int slam_v2_minimize_stage_trace(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active, const double* x0,
                                 const double* init_lo, const double* init_hi, const double* bound_lo, const double* bound_hi,
                                 const slam_opt_params* params, double exit_loss, int32_t trace_cap, double* best_loss, double* best_x,
                                 int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status, double* trace_loss,
                                 double* trace_x);

/*
 * Parallel-drive ("smush") gates -- CircuitTemplateV2(param_vec_expand=[offset, N, N]) with ConversionGainSmushGate
 * (custom_gates.py:215-257, hamiltonian.py:114-144, basisv2.py:47-50,268-273): a conversion-gain pulse with single-qubit drives
 * applied during it, cut into N time slices with their own drive amplitudes,
 *     G = U_{N-1} ... U_0,  U_s = exp(-i (t / N) H_s),
 *     H_s = gx[s] (A + A^+) + gy[s] (B + B^+) + gc (e^{i pc} A B^+ + h.c.) + gg (e^{i pg} A B + h.c.).
 * Phases pc, pg in {0, pi} only (pi flips the sign of gc / gg: fold it into the map).  A slam_smush_gate says how the raw pulse
 * values, in the order gc, gg, gx[0 .. N), gy[0 .. N) (raw index 2 + s for gx[s], 2 + N + s for gy[s]), follow from the gate's
 * n_params parameters q: raw[r] = scale[r] * q[sel[r]] + offset[r] (sel[r] = -1: the constant offset[r]); t is a constant.
 * Parameter vectors in index order: P0 .. P{6(k+1)-1}, then the n_params parameters of gate 1, gate 2, ...:
 * n = 6 (k + 1) + n_params k <= SLAM_SMUSH_MAX_N, spans 1..SLAM_SMUSH_MAX_SPAN; beyond that SLAM_ERR_UNSUPPORTED.
 * Cost kinds BasicCost and SquareCost; SLAM_COST_MAKHLIN returns SLAM_ERR_UNSUPPORTED.  One wavefront per (target, restart) item.
 *   slam_smush_set_gates               the table of smush base gates (host side only)
 *   slam_smush_eval_loss_grad          as slam_v2_eval_loss_grad (angles beyond 2e8 rad evaluate to NaN)
 *   slam_smush_minimize_stage(_trace)  as slam_v2_minimize_stage(_trace): projected quasi-Newton over the box, Philox start points in
 *                                      [init_lo, init_hi), restart-major queue, ordered early exit, lowest-index restart below exit_loss
 */
#define SLAM_SMUSH_MAX_SLICES 58
#define SLAM_SMUSH_RAW (2 + 2 * SLAM_SMUSH_MAX_SLICES)
#define SLAM_SMUSH_MAX_SPAN 6
#define SLAM_SMUSH_MAX_N 128
typedef struct slam_smush_gate {
    int32_t n_params;
    int32_t n_slices;
    double t;
    int32_t sel[SLAM_SMUSH_RAW];
    double scale[SLAM_SMUSH_RAW];
    double offset[SLAM_SMUSH_RAW];
} slam_smush_gate;
int slam_smush_set_gates(slam_ctx* ctx, const slam_smush_gate* gates, int32_t n_gates);
int slam_smush_eval_loss_grad(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x, const int32_t* target_of, int64_t M,
                              double* loss, double* grad, double* unitary);
int slam_smush_minimize_stage(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active, const double* x0,
                              const double* init_lo, const double* init_hi, const double* bound_lo, const double* bound_hi,
                              const slam_opt_params* params, double exit_loss, double* best_loss, double* best_x, int32_t* best_restart,
                              double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals);
int slam_smush_minimize_stage_trace(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active, const double* x0,
                                    const double* init_lo, const double* init_hi, const double* bound_lo, const double* bound_hi,
                                    const slam_opt_params* params, double exit_loss, int32_t trace_cap, double* best_loss, double* best_x,
                                    int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status, double* trace_loss,
                                    double* trace_x);

/*
 * Three-qubit templates, 8x8 targets (csrc/slam_q3.hpp; the reference's CircuitTemplate(n_qubits=3, edge_params=...),
 * src/slam/basis.py:52-169).  The circuit, in time order: a U3 on q0, on q1, on q2, then per two-qubit gate j = 0 .. k - 1 on the edge
 * (a_j, b_j): the gate, a U3 on a_j, a U3 on b_j.  n = 9 + 6 k parameters in index order, (theta, phi, lambda) per U3;
 * 1 <= k <= SLAM_Q3_MAX_SPAN (beyond: SLAM_ERR_UNSUPPORTED).  Matrices are qiskit little-endian 8x8, double[8][8][2] row-major, basis
 * index q0 + 2 q1 + 4 q2; a gate's 4x4 on the edge (a, b) has qubit a as its bit 0 and qubit b as its bit 1.
 * Both calls are self-contained: gates, targets and parameters come from the host with the call; the context lends its device and
 * stream, and its resident 4x4 targets, gate table, results and statistics are not touched.
 *   gates       double[n_gates][4][4][2]   the gate table
 *   gate_index  int32[k]                   the table entry of position j
 *   edges       int32[k][2]                (a_j, b_j): ordered pairs of distinct qubits from {0, 1, 2}
 *   targets     double[n_targets][8][8][2]
 *   cost_kind   SLAM_COST_BASIC  1 - |Tr(T^+ W)| / 8,  SLAM_COST_SQUARE  1 - (|Tr(T^+ W)|^2 + 8) / 72;
 *               SLAM_COST_MAKHLIN returns SLAM_ERR_UNSUPPORTED (Weyl chamber only for 2Q gates, cost_function.py)
 * slam_q3_eval: M items, item m = (x[m], target target_of[m]):
 *   x double[M][n], target_of int32[M]; out: loss double[M], grad double[M][n] (may be NULL), unitary double[M][8][8][2] (may be NULL)
 * slam_q3_minimize: one stage, as slam_minimize_stage -- for every target `restarts` quasi-Newton minimisations (one wavefront per
 * item, restart-major queue, Philox start points keyed (pair, restart, target index + target_base, k) or explicit x0, ordered early
 * exit at exit_loss); the stage result of a target is the lowest-index restart below exit_loss with SLAM_FLAG_ORDERED, the smallest
 * loss otherwise and when no restart is below it:
 *   x0 double[n_targets][R][n] or NULL (every entry finite with |x| < 1e8, as slam_minimize_stage asks of its seeds: SLAM_ERR_INVALID
 *   otherwise); out (any may be NULL): best_loss double[n_targets], best_x double[n_targets][n],
 *   best_restart int32[n_targets]; per item [n_targets][R]: item_loss, item_iters, item_status (SLAM_ST_*), item_evals,
 *   item_x double[n_targets][R][n]; kernel_ms: device time of the optimizer kernel
 * Arguments are checked before the context and before anything touches the device.
 */
#define SLAM_Q3_MAX_SPAN 15
int slam_q3_eval(slam_ctx* ctx, const double* gates, int32_t n_gates, int32_t k, const int32_t* gate_index, const int32_t* edges,
                 const double* targets, int64_t n_targets, const double* x, const int32_t* target_of, int64_t M, int32_t cost_kind,
                 double* loss, double* grad, double* unitary);
int slam_q3_minimize(slam_ctx* ctx, const double* gates, int32_t n_gates, int32_t k, const int32_t* gate_index, const int32_t* edges,
                     const double* targets, int64_t n_targets, int32_t cost_kind, const slam_opt_params* params, double exit_loss,
                     const double* x0, double* best_loss, double* best_x, int32_t* best_restart, double* item_loss, int32_t* item_iters,
                     int32_t* item_status, int32_t* item_evals, double* item_x, double* kernel_ms);

/*
 * Mixed templates: positions that hold a three-qubit gate (the reference's `circuit.append(gate, edge)` with an edge of three qubits,
 * src/slam/basis.py:152-169; its CirculatorSNAILGate, VSwap, DeltaSwap, CCZGate, Peres ...).  A position of arity 3 on the ordered
 * triple (a, b, c) -- all three qubits; gate-local bit 0 is qubit a, bit 1 is b, bit 2 is c -- is the gate, then a U3 on a, on b, on c;
 * a position of arity 2 is as above.  n = 9 + 3 * sum(arity_j) parameters, in circuit order.  Caps: 1 <= k <= SLAM_Q3_MAX_SPAN,
 * n <= 99 and n_gates3 <= SLAM_Q3_MAX_GATES3 distinct three-qubit gates (the kernel keeps one 1 KB table per distinct gate in LDS);
 * beyond any of them: SLAM_ERR_UNSUPPORTED.
 *   gates2      double[n_gates2][4][4][2]  the two-qubit gate table (n_gates2 may be 0, gates2 NULL then)
 *   gates3      double[n_gates3][8][8][2]  the three-qubit gate table, basis index bit_a + 2 bit_b + 4 bit_c (n_gates3 may be 0)
 *   arity       int32[k]                   2 or 3
 *   gate_index  int32[k]                   the entry of position j in the table of its arity
 *   qubits      int32[k][3]                (a_j, b_j, c_j): distinct qubits from {0, 1, 2}; c_j is ignored at arity 2
 * Everything else is as in slam_q3_eval / slam_q3_minimize (the Philox key keeps k, the number of positions).  A template without a
 * position of arity 3 runs the kernels of that pair and returns bit for bit what it returns; the mixed kernel instantiations
 * run only when a position has arity 3.  Arguments are checked before the context and before anything touches
 * the device.
 */
#define SLAM_Q3_MAX_GATES3 3
int slam_q3m_eval(slam_ctx* ctx, const double* gates2, int32_t n_gates2, const double* gates3, int32_t n_gates3, int32_t k, const int32_t* arity,
                  const int32_t* gate_index, const int32_t* qubits, const double* targets, int64_t n_targets, const double* x,
                  const int32_t* target_of, int64_t M, int32_t cost_kind, double* loss, double* grad, double* unitary);
int slam_q3m_minimize(slam_ctx* ctx, const double* gates2, int32_t n_gates2, const double* gates3, int32_t n_gates3, int32_t k,
                      const int32_t* arity, const int32_t* gate_index, const int32_t* qubits, const double* targets, int64_t n_targets,
                      int32_t cost_kind, const slam_opt_params* params, double exit_loss, const double* x0, double* best_loss, double* best_x,
                      int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals, double* item_x,
                      double* kernel_ms);

/*
 * State objectives of the three-qubit templates (the reference's EntanglementCostFunction, src/slam/cost_function.py:44-99, the second
 * branch of its objective, src/slam/optimizer.py:203-205): a start state psi -- 8 amplitudes, basis index q0 + 2 q1 + 4 q2, of unit norm
 * -- goes through the template, v = W(x) psi, and the loss is the entanglement left in v, in bits:
 *   SLAM_COST_MUTUAL_INFO         I(1:2) + I(0:2) + I(0:1),  I(a:b) = S(rho_a) + S(rho_b) - S(rho_ab)   (MutualInformation)
 *   SLAM_COST_MUTUAL_INFO_SQUARE  the sum of the three squares                                        (MutualInformationSquare)
 * Both are zero exactly on product states.  The template description, the caps, the Philox keying (a state's index takes the
 * target's place), the ordered early exit, the outputs and kernel_ms are those of slam_q3m_eval / slam_q3m_minimize; a template
 * without a position of arity 3 runs the non-mixed kernel.
 *   states      double[n_states][8][2]     every entry finite, | |psi|^2 - 1 | <= 1e-9 (SLAM_ERR_INVALID otherwise)
 *   state_of    int32[M]                   the state of item m
 *   cost_kind   one of the two above; anything else, SLAM_COST_BASIC / SQUARE / MAKHLIN included: SLAM_ERR_INVALID
 *   out_state   double[M][8][2]            v of every item (may be NULL)
 * Loss and gradient are finite for every such state and every finite x: where a reduced state is maximally mixed the derivative is
 * taken from its series, and a qubit whose reduced state is pure to rounding contributes zero to both.
 * Arguments are checked before the context and before anything touches the device.  slam_set_cost does not take these kinds.
 */
#define SLAM_COST_MUTUAL_INFO 3
#define SLAM_COST_MUTUAL_INFO_SQUARE 4 /* accepted by the two calls below only */
int slam_q3s_eval(slam_ctx* ctx, const double* gates2, int32_t n_gates2, const double* gates3, int32_t n_gates3, int32_t k, const int32_t* arity,
                  const int32_t* gate_index, const int32_t* qubits, const double* states, int64_t n_states, const double* x,
                  const int32_t* state_of, int64_t M, int32_t cost_kind, double* loss, double* grad, double* out_state);
int slam_q3s_minimize(slam_ctx* ctx, const double* gates2, int32_t n_gates2, const double* gates3, int32_t n_gates3, int32_t k,
                      const int32_t* arity, const int32_t* gate_index, const int32_t* qubits, const double* states, int64_t n_states,
                      int32_t cost_kind, const slam_opt_params* params, double exit_loss, const double* x0, double* best_loss, double* best_x,
                      int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals, double* item_x,
                      double* kernel_ms);

/*
 * Hamiltonian templates (csrc/slam_ham.hpp; the reference's HamiltonianTemplate, src/slam/basis.py:24-48, over src/slam/hamiltonian.py):
 * the parameters x are the drive strengths and phases (and possibly the time) of
 *   H(x) = sum_k c_k M_k + h.c.,   c_k = x[s_index[k]] exp(i x[phi_index[k]])   (phi_index[k] = -1: phase 0),
 * and the template's unitary is exp(-i t H(x)), t = x[t_index] (t_index = -1: t = 1).  dim is 4 or 8; matrices are row-major.
 *   matrices    double[n_terms][dim][dim][2]   the M_k; n_terms <= SLAM_HAM_MAX_TERMS, n_params <= SLAM_HAM_MAX_PARAMS, and no entry of
 *                                              H may take more than two contributions (beyond any of them: SLAM_ERR_UNSUPPORTED)
 *   s_index     int32[n_terms]                 in 0 .. n_params - 1
 *   phi_index   int32[n_terms]                 in -1 .. n_params - 1
 *   targets     double[n_targets][dim][dim][2] any finite matrices (they need not be unitary)
 *   cost_kind   SLAM_COST_BASIC  1 - |Tr(T^+ U)| / dim,  SLAM_COST_SQUARE  1 - (|Tr(T^+ U)|^2 + dim) / (dim (dim + 1)); others:
 *               SLAM_ERR_INVALID
 * slam_ham_eval: M items, item m = (x[m], target target_of[m]); x double[M][n_params], every entry finite; out: loss double[M],
 *   grad double[M][n_params] (may be NULL), unitary double[M][dim][dim][2] (may be NULL).
 * slam_ham_minimize: one stage as slam_q3_minimize -- the same quasi-Newton iteration, status codes, restart-major queue, ordered
 *   early exit at exit_loss, reduction over the restarts, outputs and kernel_ms -- except that x0 double[n_targets][R][n_params] is
 *   REQUIRED (every entry finite with |x| < 1e8): the start points are drawn on the host, the device draws none.
 * Both calls are self-contained (nothing of the context is touched or kept), and dimensions, index arrays, caps, matrices, targets,
 * start points and the cost kind are checked before the context and before anything touches the device.
 */
#define SLAM_HAM_MAX_TERMS 16
#define SLAM_HAM_MAX_PARAMS 32
int slam_ham_eval(slam_ctx* ctx, int32_t dim, int32_t n_params, int32_t n_terms, const double* matrices, const int32_t* s_index,
                  const int32_t* phi_index, int32_t t_index, const double* targets, int64_t n_targets, const double* x, const int32_t* target_of,
                  int64_t M, int32_t cost_kind, double* loss, double* grad, double* unitary);
int slam_ham_minimize(slam_ctx* ctx, int32_t dim, int32_t n_params, int32_t n_terms, const double* matrices, const int32_t* s_index,
                      const int32_t* phi_index, int32_t t_index, const double* targets, int64_t n_targets, int32_t cost_kind,
                      const slam_opt_params* params, double exit_loss, const double* x0, double* best_loss, double* best_x, int32_t* best_restart,
                      double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals, double* item_x, double* kernel_ms);

/*
 * Time-sliced Hamiltonian templates (csrc/slam_hams.hpp; the reference's ConversionGainSmush / ConversionGainSmush1QPhase,
 * src/slam/hamiltonian.py:114-182): a piecewise-constant pulse of n_slices slices of equal length,
 *   U(x) = U_S ... U_2 U_1,   U_s = exp(-i (t / S) H_s(x)),   H_s(x) = sum_k c_{s,k} M_k + h.c.,
 *   c_{s,k} = x[s_index[s][k]] exp(i x[phi_index[s][k]])   (phi_index[s][k] = -1: phase 0),   t = x[t_index] (t_index = -1: t = 1);
 * slice 0 acts first.  The term matrices are shared by the slices; a parameter may feed one slice, several or all of them.
 * slam_hams_eval and slam_hams_minimize are slam_ham_eval and slam_ham_minimize -- arguments, checks before the context, outputs,
 * status codes, ordered early exit and reduction over the restarts -- with
 *   n_slices    in 1 .. SLAM_HAMS_MAX_SLICES (0 and below: SLAM_ERR_INVALID; above: SLAM_ERR_UNSUPPORTED)
 *   s_index     int32[n_slices][n_terms]       in 0 .. n_params - 1
 *   phi_index   int32[n_slices][n_terms]       in -1 .. n_params - 1
 * and one difference in what a slice's Hamiltonian may hold: the two halves (M and its adjoint) of a phase-free term on a DIAGONAL entry
 * count as one contribution of weight 2 Re M[r][r], so that two number operators may share an entry; the limit of two contributions
 * per entry holds per slice.  n_slices = 1 computes what the slam_ham_* pair computes.
 */
#define SLAM_HAMS_MAX_SLICES 8
int slam_hams_eval(slam_ctx* ctx, int32_t dim, int32_t n_params, int32_t n_terms, int32_t n_slices, const double* matrices, const int32_t* s_index,
                   const int32_t* phi_index, int32_t t_index, const double* targets, int64_t n_targets, const double* x, const int32_t* target_of,
                   int64_t M, int32_t cost_kind, double* loss, double* grad, double* unitary);
int slam_hams_minimize(slam_ctx* ctx, int32_t dim, int32_t n_params, int32_t n_terms, int32_t n_slices, const double* matrices,
                       const int32_t* s_index, const int32_t* phi_index, int32_t t_index, const double* targets, int64_t n_targets, int32_t cost_kind,
                       const slam_opt_params* params, double exit_loss, const double* x0, double* best_loss, double* best_x, int32_t* best_restart,
                       double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals, double* item_x, double* kernel_ms);

/*
 * Multi-GPU: one process per GPU, RCCL over xGMI, reached through this ABI (no torch, no MPI).  The path shards by
 * target, every rank keeps all restarts of its targets, so the only exchange is the FINAL min-all-reduce of the
 * best-loss vector -- the running minimum of TemplateOptimizer._run (src/slam/optimizer.py:281-284) taken over the
 * ranks -- plus a few scalars (barrier, slowest rank's time, counts).  librccl.so is dlopen'ed by the first of these
 * calls; a single-GPU process never loads it.
 *   slam_comm_get_unique_id   rank 0 creates the 128-byte id and hands it to the other ranks (file, env, socket:
 *                             the caller's business; bench.py / parallel.py use a file)
 *   slam_comm_init            ncclCommInitRank on `device` (collective: every rank calls it with the same id)
 *   slam_comm_allreduce_f64   in-place all-reduce of a small host array (staged through device memory)
 *   slam_comm_barrier         all ranks have arrived
 *   slam_comm_merge_begin     start a job-wide best-loss vector of n_global entries on this rank's GPU, all +inf
 *   slam_comm_merge_add       min-merge the context's RESIDENT best_loss[first_local, first_local + count) -- the
 *                             buffer slam_best_loss_device_ptr exposes -- into [first_global, first_global + count)
 *                             of that vector, device to device (call once per context / window of the rank).  The
 *                             context must live on the communicator's device (SLAM_ERR_INVALID otherwise); the read of
 *                             its buffer is complete when the call returns, so the context may be used again at once
 *   slam_comm_merge_add_host  the same from a host array (results that were fetched already)
 *   slam_allreduce_min        ncclAllReduce(min) of the vector in place over xGMI; n_below (may be NULL) = number of
 *                             entries < threshold counted on the device, merged (may be NULL) = host copy of the
 *                             n_global entries, merged_capacity = doubles it can hold (SLAM_ERR_INVALID if fewer)
 *   slam_comm_rank            rank / world size as RCCL ITSELF reports them (ncclCommUserRank / ncclCommCount);
 *                             SLAM_ERR_STATE if they differ from what slam_comm_init was given
 */
#define SLAM_COMM_ID_BYTES 128
#define SLAM_OP_SUM 0
#define SLAM_OP_MAX 2
#define SLAM_OP_MIN 3
typedef struct slam_comm slam_comm;
int slam_comm_get_unique_id(void* id);
int slam_comm_init(int device, int rank, int world, const void* id, slam_comm** out);
int slam_comm_destroy(slam_comm* comm);
int slam_comm_rank(slam_comm* comm, int* rank, int* world);
int slam_comm_allreduce_f64(slam_comm* comm, double* inout, int64_t n, int op);
int slam_comm_barrier(slam_comm* comm);
int slam_comm_merge_begin(slam_comm* comm, int64_t n_global);
int slam_comm_merge_add(slam_comm* comm, slam_ctx* ctx, int64_t first_local, int64_t count, int64_t first_global);
int slam_comm_merge_add_host(slam_comm* comm, const double* loss, int64_t count, int64_t first_global);
int slam_allreduce_min(slam_comm* comm, double threshold, int64_t* n_below, double* merged, int64_t merged_capacity);

/*
 * Hardware queues.  The HIP runtime maps all streams of a process onto GPU_MAX_HW_QUEUES hardware queues (its default: 4) and reads
 * that variable once, at its first call; streams that share a queue serialise, so contexts that are meant to run side by side --
 * several calls in flight from host threads, the helper streams of speculative / overlapped spans -- need one queue each.  The
 * library asks for them itself: a load-time initialiser (before any HIP call of the library) sets GPU_MAX_HW_QUEUES to 16 when it is
 * unset, not a number or below 16.  A value of 16 or more is kept: the variable is never lowered, and nothing above 32 is ever
 * written.  SLAM_HW_QUEUES=0 in the environment switches the initialiser off, SLAM_HW_QUEUES=N (4 <= N <= 32) asks for N instead of
 * 16; any other value is ignored.  A process that has initialised HIP BEFORE it loads the library is out of its reach: there the
 * caller exports the variable, as before.
 * Returns the value of GPU_MAX_HW_QUEUES in force after the initialiser ran, or 0 when it was switched off.
 */
int slam_hw_queues_requested(void);

/* Library version string. */
const char* slam_version(void);

/* Binary interface revision: bumped whenever an exported function changes its signature or a structure its layout.  History:
 *   4  slam_allreduce_min took its fifth argument, merged_capacity (round 3, without a new symbol: a caller built against an older
 *      header must check the revision before calling);
 *   5  round 4: slam_decompose_multi, slam_predict_spans, 32-byte item records;
 *   6  round 5: SLAM_MAX_SPAN_EVAL / SLAM_MAX_SPAN_MINIMIZE 5 -> 16 -- the per-span arrays of slam_stats and the rows of
 *      slam_fetch_span_losses grow with them --, SLAM_FLAG_NO_EXTERIOR, kernel_ms_span[0];
 *   7  round 5: slam_host_alloc / slam_host_free (new symbols only);
 *      later: slam_coverage_lookup (a new symbol only; no signature or structure changed);
 *      later: the slam_smush_* family and its own slam_smush_gate (new symbols only);
 *      later: slam_pd_sample, slam_pd_extremes, slam_pd_filter and slam_region_lookup (new symbols only);
 *      later: slam_hw_queues_requested (a new symbol only);
 *      later: slam_kak, slam_targets_kak and slam_complete_locals (new symbols only);
 *      later: slam_metric_update_check (a new symbol only);
 *      later: slam_haar_select_spans and slam_sample_haar_indexed (new symbols only);
 *      later: slam_sqiswap_decompose (a new symbol only);
 *      later: slam_cx_decompose (a new symbol only);
 *      later: slam_b_decompose (a new symbol only);
 *      later: slam_family_lookup (a new symbol only);
 *      later: slam_approx_decompose and slam_approx_counts (new symbols only);
 *      later: slam_candidate_scores (a new symbol only);
 *      later: slam_sc_decompose and slam_sc_counts (new symbols only);
 *      later: slam_sqiswap_approx_decompose and slam_sqiswap_approx_counts (new symbols only);
 *      later: slam_q3_eval and slam_q3_minimize (new symbols only);
 *      later: slam_q3m_eval and slam_q3m_minimize (new symbols only);
 *      later: slam_q3s_eval and slam_q3s_minimize (new symbols only);
 *      later: slam_ham_eval and slam_ham_minimize (new symbols only);
 *      later: slam_hams_eval and slam_hams_minimize (new symbols only).
 * The Python binding refuses a library whose revision differs from the one it was written for. */
#define SLAM_ABI_VERSION 7
int slam_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SLAM_HIP_H */
