// qpb_gi.hip -- batched dense active-set QP kernel for gfx950 (n <= 16).
//
//   min 1/2 x^T H x + f^T x   s.t.   A x <= b        (fp64, one QP per 16 lanes)
//
// Replaces, batched, the reference's hot path: the dense kernels of
// matrix/matrix_ops/matrix_ops.c (matrix_mult GEMV :235-271, LU/inverse
// :487-630, vector ops :158-411, norm :632-656) driving the solver iterations
// of qp_solvers/qp_solvers.c.  The constrained iteration north_star asks for
// (absent from the reference) is the dual active-set method of
// Goldfarb & Idnani (Math. Prog. 27, 1983), which needs no feasible start:
//
//   setup   H = L L^T, D = A L^{-T}, y = L^{-1} f in ONE right-looking sweep:
//           step k broadcasts pivot row k of the Schur complement (DPP
//           row_newbcast from lane k); by symmetry it is also column k, so
//           the same broadcast drives the Schur update of row l (lane l), the
//           substitution of both D rows of lane l and the lane-parallel y.
//           Slack of the unconstrained minimiser x0 = -H^{-1} f
//           (test/qp_ref.py:35's answer): s = b - A x0 = b + D y.
//   iterate D = A L^{-T} Q is kept in the rotated basis Q: the rows of the
//           active constraints are zero on the free basis columns q..15.
//           Pick the violated row p with the largest violation per unit
//           length of its free part, -s_p / |D[p, q:]| (dual steepest edge;
//           the squared free norms are kept up to date, fp32 keys); its row
//           d = D[p,:] splits into d1 (columns < q) and d2 (columns >= q).
//           Dual step r = R^{-1} d1 (lane-parallel back substitution over the
//           prefetched R column), partial step t1 (ratio test over the active
//           multipliers), full step t2 = -s_p / |d2|^2, slacks s -= t D d2.
//           full step  -> ADD p: one Householder reflection on columns q..15
//                         of D (every lane updates its own rows; its product
//                         D v = D d2 + alpha D[:, q] reuses the slack step's
//                         D d2 and reads column q by a branch tree on q), new
//                         column of R;
//           partial    -> DROP k: delete column k of R, Givens rotations
//                         restore triangularity (also applied to D).
//   finish  x = -H^{-1} (f + A^T lam) from the final multipliers (KKT
//           stationarity): the active rows of A are re-read, two lane-
//           parallel triangular solves with L kept in LDS.
//
// Data layout per QP (lane l = 0..15 of the QP's 16-lane DPP row):
//   registers  rows l + 16 r (r < MR) of D, their slacks, their violation
//              thresholds (the high word is a NaN's while the row is active,
//              with a copy to put back), |D row|^2, |free part|^2; multiplier / row of
//              active position l, R[l][l] and its reciprocal; in a DROP the
//              parameters of Givens rotation l
//   LDS        L (packed rows), R (16 x 16 column-major, zero diagonal; its
//              column 0 carries the exchange row).  The whole slot is the staging buffer of the
//              coalesced input transposes before the factorisation, and the
//              dead R holds the lambda scatter and the x capture after the
//              loop.
// Every product with a vector held one entry per lane (d2, the Householder
// vector) is a v_fmac_f64_dpp reading the entry from lane j by row_newbcast:
// no LDS round trip, no copy of the vector in every lane.
// No branch or select compares the lane id with a compile-time constant:
// such masks are hoisted by the compiler and end up spilled (SGPR pressure).
#include "qpb_factor.h"  // the factor buffer of qpb_factor_shared / qpb_solve_factored
#include "qpb_launch.h"  // with qpb.h
#include "qpb_row16.h"   // the QP's LDS slot and the steps shared with gi_box and kkt_bwd

namespace qpb {
using namespace row16;

// out[r] = sum_j vec[lane j] * x[r][j] over the row's 16 lanes, DPP-fused;
// the MR rows interleaved, two chains each (2 MR independent accumulators);
// the caller has issued dpp_ready(vec)
template <int MR>
__device__ __forceinline__ void bdot_rows(double vec, const double (&x)[MR][NL], double (&out)[MR]) {
  double a[MR][2];
#pragma unroll
  for (int r = 0; r < MR; ++r) a[r][0] = a[r][1] = 0.0;
  unroll<NL>([&](auto J) {
    constexpr int j = J;
#pragma unroll
    for (int r = 0; r < MR; ++r) fmac_bc<j>(a[r][j & 1], vec, x[r][j]);
  });
#pragma unroll
  for (int r = 0; r < MR; ++r) out[r] = a[r][0] + a[r][1];
}

// The high word of a double, and the double with that word replaced (the low
// word kept): sub-register moves, no arithmetic
__device__ __forceinline__ uint32_t hi32(double v) {
  return (uint32_t)(__builtin_bit_cast(unsigned long long, v) >> 32);
}
__device__ __forceinline__ double with_hi32(double v, uint32_t hi) {
  const unsigned long long lo = __builtin_bit_cast(unsigned long long, v) & 0xFFFFFFFFull;
  return __builtin_bit_cast(double, lo | ((unsigned long long)hi << 32));
}
// The high word a row's threshold carries while the row is in the active set:
// a quiet NaN, so the selection's s < thr is false for it
constexpr uint32_t kActiveHi = 0x7FF80000u;

// MR: rows of D per lane (m <= 16 MR).  N16: n == 16 (coalesced loads).
// FULL: n == 16 and m == 16 MR (no padding rows: no masking anywhere).
// One group = the 4 QPs of a wavefront; `grp` its index.
// EQ (qpb_solve_eq): rows 0 .. meq-1 are equalities a x = b.  They enter the
// active set first, in index order, and never leave it: row p's sign is
// chosen when it is selected (s_p > 0: row p of D and s_p are negated in
// place, the position remembers it), after which it is an ordinary violated
// row with s_p <= 0 and a free multiplier.  They hold the active positions
// 0 .. eqs.q-1, which the ratio test leaves out, so a DROP never touches them.
// A row that depends on the equalities before it is left out (bit clear,
// lam = 0) when its residual is within the tolerance, else the QP is
// INFEASIBLE.  The finish writes lam and x with the caller's signs.
// SH (qpb_solve_shared): the QP strides of H and A, in doubles, are the
// run-time strideH and strideA -- 0 for an operand the whole batch shares, or
// n n and m n -- in every address that reads H or A; the arithmetic is the
// other forms', so the outputs are theirs bit for bit.  Without SH the two
// arguments are unused and every address is formed as before.
// RG (qpb_solve_range, on EQ and SH): rows meq .. m-1 are two-sided,
// bl <= a x <= bu, with bg = bu and blg = bl (either may be NULL: that side is
// absent everywhere).  Only one side of a row can be active, so the lane holds
// one side at a time: a bit per row says that its row of D and its slack are
// the negated, lower-side ones (s = a x - bl), and w = bu - bl turns one
// side's slack into the other's, w - s.  A row is selected on the side that
// is violated; if that is not the side held, the owner negates the row and
// its slack in place first -- what the EQ phase does for s_p > 0.  The active
// position remembers the side (pneg travels with um and iam through a DROP),
// the multiplier changes sign once at the end, and `lowg` gets the rows
// active at their lower bound.  The norms (thr, ddr, fn2) do not depend on
// the side.  A dropped row keeps its side; its slack follows the updates like
// any inactive row's, and it can come back on either side.
// BX (qpb_solve_range_box, on RG): the last n of the m rows are the variables'
// bounds, row mg + j being lb_j <= x_j <= ub_j (ubg, lbg: n per QP, either may
// be NULL); bg, blg and Ag hold the mg rows before them only.  A lane's row
// l + 16 r sits where the materialised [G; I] would put it; a row >= mg is
// e_{row - mg} made in registers -- no address of G is formed for it in any of
// the three load paths -- row_norms runs on it unchanged, so the thresholds are
// the materialised form's bits, and in the x recovery its position adds
// um e_j.  Everything between is the RG form's code.
// FM (qpb_factor_shared and qpb_solve_factored; qpb_factor.h has the buffer):
//   1  the factor kernel's body: ONE problem (batch 1, no f and no b), this
//      form's own load and sweep, then L, D, the rows' norms, A and what the
//      set-up found go to the buffer `xg` (and the finding to statg, if given),
//      and nothing else runs
//   2  the factored solve, on SH with both strides 0: Hg is the buffer and Ag
//      its copy of A.  No H or A is loaded and nothing is staged: the lane's row
//      of L and its MR rows of D come from the buffer, thr from the stored |a_r|,
//      ddr and fn2 from the stored |D_r|^2; then y = L^-1 f by a lane-parallel
//      forward substitution and s = b + D y, n (1 + MR) DPP-fused FMAs in place
//      of the sweep.  From there on -- the loop and the outputs -- the code is
//      the other forms', plain and EQ.
//      With RG (qpb_solve_range_factored): bu and bl are loaded as in the range
//      form; row_norms takes |a_r|^2 and |a_r| from the buffer, so the thresholds
//      are the unfactored range form's bit for bit, and a row whose only bound
//      is the lower one negates the lane's row of D -- the negated row of A would
//      have swept into exactly that -- before s is formed.  The loop and the
//      outputs are the range form's.
#ifdef QPB_WAVE_TRACE
// diagnostic build only (tools/wave_timeline.py): the low 32 bits of the
// 100 MHz real-time counter into 32-bit word w (12 .. 15: the record's free
// words 6 and 7) of the group's 8-word record
__device__ __forceinline__ void wave_stamp32(unsigned long long *dbg, long long grp, int w) {
  if (!dbg) return;
  unsigned long long t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  if (threadIdx.x == 0) reinterpret_cast<uint32_t *>(dbg)[16ull * grp + w] = (uint32_t)t;
}
#endif

template <int MR, bool N16, bool FULL, bool STAMP, bool EQ = false, bool SH = false, bool RG = false, int FM = 0,
          bool BX = false>
__device__ __forceinline__ void gi_group(
    double *lds, const double *__restrict__ Hg, const double *__restrict__ fg, const double *__restrict__ Ag,
    const double *__restrict__ bg, double *__restrict__ xg, double *__restrict__ lamg,
    uint32_t *__restrict__ actg, int32_t *__restrict__ statg, int32_t *__restrict__ itg, int n, int m,
    long long batch, int max_iter, double feas_tol, int flags, unsigned long long *__restrict__ dbg,
    long long grp, [[maybe_unused]] int meq = 0, [[maybe_unused]] long long strideH = 0,
    [[maybe_unused]] long long strideA = 0, [[maybe_unused]] const double *__restrict__ blg = nullptr,
    [[maybe_unused]] uint32_t *__restrict__ lowg = nullptr, [[maybe_unused]] int mg = 0,
    [[maybe_unused]] const double *__restrict__ ubg = nullptr, [[maybe_unused]] const double *__restrict__ lbg = nullptr) {
  static_assert(!FULL || N16, "FULL implies n == 16");
  static_assert(!BX || (RG && FM == 0), "the box rows are the unfactored range form's");
  static_assert(!RG || (EQ && SH), "the range form is built on the EQ and the shared forms");
  static_assert(!SH || !STAMP, "the shared form has no stamped build");
  static_assert(FM == 0 || (!STAMP && (FM == 1 ? !EQ && !SH && !RG : SH)),
                "the factor forms are plain, EQ or SH ones; the range form has a factored solve only");
  SectionClock<STAMP> clk;
  const int l = threadIdx.x & (NL - 1);
  const int slot = threadIdx.x >> 4;
  const int sh = (threadIdx.x & 63) & ~(NL - 1);  // this row's bit offset in a wave ballot
  // Rows past the end of the batch (last group only) do not leave: they replay
  // the batch's last QP -- same trip count, so they never extend the wave's
  // loop -- and store nothing.  Every lane of the wave stays live, so the
  // cross-row reads (wave_max4's readlanes) only ever see real QP state.
  // The group's first QP, g0 = 4 grp, is wave-uniform and so is every base
  // address below; a lane adds a 32-bit byte offset inside the group's block
  // (under 16 KiB: 4 QPs of m <= 32 rows of n <= 16 doubles).  `rem` QPs of the
  // group exist (batch - 1 >= g0, so a replaying row's index rem - 1 is in 0..3).
  const long long g0 = grp * QPB;
  const int rem = (int)__builtin_elementwise_min(batch - g0, (long long)QPB);
  const bool live = slot < rem;
  const uint32_t sl = (uint32_t)(live ? slot : rem - 1);  // this row's QP inside the group
  if constexpr (FULL) {
    n = NL;
    m = NL * MR;
    if constexpr (BX) mg = NL * (MR - 1);
  }

  double *base = slot_base(lds, slot);
  double *Lp = base + OFF_L;
  double *Tv = base + OFF_R;  // R, column-major (zero diagonal)
  // the exchange row in R's column 0: the back substitution never reads that
  // column, a DROP rebuilds it before use, an ADD at q = 0 rewrites it
  double *xch = Tv;
  double *xsd = base + OFF_XCH;  // s_p, |D[p,:]|^2

  // ------------------------------------------------------------------ load
  // (flags & QPB_FLAG_DIAG_L2: every QP reads the inputs of QP g mod 512;
  // QPB_FLAG_DIAG_MALL: of QP g mod 16384 (107 MB, Infinity-Cache resident
  // after the first launch) -- diagnostics that take HBM out of the kernel time)
  // (512 and 16384 are multiples of 4: the group's four indices never wrap,
  // the masked index of its first QP serves all of them)
  const long long gi0 = (flags & QPB_FLAG_DIAG_L2) ? (g0 & 511) : (flags & QPB_FLAG_DIAG_MALL) ? (g0 & 16383) : g0;
  const double *Hs = SH ? Hg + gi0 * strideH : Hg + gi0 * (long long)n * n;
  // m == 0: A/b may be NULL -- point the (masked) row loads at H instead
  // (BX: the same for mg == 0, and no load goes through As then)
  const double *As = (BX ? mg : m) > 0 ? (SH ? Ag + gi0 * strideA : Ag + gi0 * (long long)m * n) : Hs;
  const double *bs = m > 0 ? bg + gi0 * (long long)m : Hs;
  const uint32_t un = (uint32_t)n, umn = (uint32_t)m * un;
  double Lr[NL];  // row l of H, becomes row l of L
  double E[MR][NL];
  double s[MR], bl[MR], thr[MR];
  float ddr[MR];  // |D[r,:]|^2 (the dependency test's scale; clamped to FLT_MAX)
  float fn2[MR];  // |D[r, q:]|^2, the free part of the row (scale of the selection key)
  // The active flag of a row lives in thr: the high word is kActiveHi while the
  // row is in the active set, and thh keeps the word to put back at a DROP
  uint32_t thh[MR];
  bool infeasible_row = false;
  // b and f with the matrices (same round trip)
  double bv[MR];
  [[maybe_unused]] RgState<RG, MR> rg;
  // FM: per row |a_r|^2 and |a_r| (1: found by row_norms; 2: from the buffer)
  [[maybe_unused]] double an2[MR], an1[MR];
  if constexpr (FM == 1) {
#pragma unroll
    for (int r = 0; r < MR; ++r) bv[r] = 0.0;
  } else if constexpr (BX) {
    // rows < mg: bu and bl at the row, mg per QP; rows mg + j: ub and lb at j, n
    // per QP.  Each of the four NULL (wave-uniform) when nothing has that side;
    // a lane whose rows are not of an array's kind reads its element 0
    const double *hi_r = bg && mg > 0 ? bg + gi0 * (long long)mg : nullptr;
    const double *lo_r = blg && mg > 0 ? blg + gi0 * (long long)mg : nullptr;
    const double *hi_b = ubg ? ubg + gi0 * n : nullptr, *lo_b = lbg ? lbg + gi0 * n : nullptr;
    unroll<MR>([&](auto R) {
      constexpr int r = R;
      const int row = l + NL * r;
      if constexpr (FULL && r < MR - 1) {  // general rows only
        const uint32_t off = (sl * (uint32_t)mg + (uint32_t)row) * 8u;
        bv[r] = hi_r ? at_off<double>(hi_r, off) : kInf;
        rg.lo[r] = lo_r ? at_off<double>(lo_r, off) : -kInf;
      } else if constexpr (FULL) {  // the variables' rows only
        const uint32_t off = (sl * un + (uint32_t)l) * 8u;
        bv[r] = hi_b ? at_off<double>(hi_b, off) : kInf;
        rg.lo[r] = lo_b ? at_off<double>(lo_b, off) : -kInf;
      } else {
        const bool gen = row < mg;
        const uint32_t offr = (sl * (uint32_t)mg + (uint32_t)(gen ? row : 0)) * 8u;
        const uint32_t offb = (sl * un + (uint32_t)((!gen && row < m) ? row - mg : 0)) * 8u;
        const double ur = hi_r ? at_off<double>(hi_r, offr) : kInf, ub = hi_b ? at_off<double>(hi_b, offb) : kInf;
        const double lr = lo_r ? at_off<double>(lo_r, offr) : -kInf, lb = lo_b ? at_off<double>(lo_b, offb) : -kInf;
        bv[r] = gen ? ur : ub;
        rg.lo[r] = gen ? lr : lb;
      }
    });
  } else if constexpr (RG) {
    // bu and bl, each NULL (wave-uniform) when no row has that side
    const double *lo_s = blg ? blg + gi0 * (long long)m : nullptr;
#pragma unroll
    for (int r = 0; r < MR; ++r) {
      const uint32_t off = (sl * (uint32_t)m + (uint32_t)((FULL || l + NL * r < m) ? l + NL * r : 0)) * 8u;
      bv[r] = bg ? at_off<double>(bs, off) : kInf;
      rg.lo[r] = lo_s ? at_off<double>(lo_s, off) : -kInf;
    }
  } else {
#pragma unroll
    for (int r = 0; r < MR; ++r)
      bv[r] = at_off<double>(bs, (sl * (uint32_t)m + (uint32_t)((FULL || l + NL * r < m) ? l + NL * r : 0)) * 8u);
  }
  double fv = 0.0;
  if constexpr (FM != 1) fv = at_off<double>(fg + gi0 * n, (sl * un + (uint32_t)(l < n ? l : n - 1)) * 8u);
  const double fl = (N16 || l < n) ? fv : 0.0;
  [[maybe_unused]] const int hr = l >> 3, hc = 2 * (l & 7);
  // stage 16 rows of a 16-column matrix (as loaded) in this QP's slot (L and
  // R are written after the factorisation)
  auto stage = [&](const double2 (&v)[8]) {
    wave_lds_sync();
#pragma unroll
    for (int t = 0; t < 8; ++t) *reinterpret_cast<double2 *>(&base[(2 * t + hr) * RS + hc]) = v[t];
    wave_lds_sync();
  };
  // row r's constant data from its entries: the violation threshold of the
  // slack, s / |a| < -tol (1 + |b| / |a|), i.e. s < -tol (|a| + |b|) (-inf: a
  // zero row, never selected), and the zero row's own test 0 <= b.  A NaN b is
  // an absent row, b = +inf (qpb.h), so the threshold is NaN exactly for a row
  // with a NaN entry or an overflowing norm (nrm2 NaN or inf, neither <= 0):
  // such a row would fail every comparison and drop out of the problem
  // unnoticed; it ends the QP as QPB_NUMERICAL before the loop instead.  The
  // flag is read back from thr[] there (thr must stay NaN-free for every other
  // input): a bool of its own, live across the factorisation sweep as in
  // gi_wave and gi_gram, cost 168 VGPRs instead of 162 at MR = 2 and 12 bytes
  // of scratch in the n = 16, m < 32 form
  auto row_norms = [&](int r, const double (&row)[NL]) {
    double nrm2;
    if constexpr (FM == 2) nrm2 = an2[r];
    else nrm2 = dot2<NL>([&](int j) { return row[j]; }, [&](int j) { return row[j]; });
    if constexpr (FM == 1) {
      an2[r] = nrm2;
      an1[r] = !(nrm2 <= 0.0) ? nrm2 * rsq1(nrm2) : 0.0;
    }
    const bool ok = FULL || l + NL * r < m;
    if constexpr (RG) {
      // A non-finite bound is an absent side (a NaN, and +-inf of either sign:
      // in the pair form a row with b = -inf is never violated either).  A row
      // whose only bound is the lower one is held lower-oriented from here on
      // (w - s would be inf - inf).  One threshold for both sides, with the
      // larger finite |bound|; crossed bounds beyond it and a zero row with 0
      // outside [bl, bu] end the QP as QPB_INFEASIBLE before the loop.  The
      // lower bound of an equality is not looked at.
      const bool eqr = ok && l + NL * r < meq;
      const bool has_hi = __builtin_fabs(bv[r]) < kInf, has_lo = !eqr && __builtin_fabs(rg.lo[r]) < kInf;
      const double hi = has_hi ? bv[r] : kInf, lo = has_lo ? rg.lo[r] : -kInf;
      const double beta = __builtin_fmax(has_hi ? __builtin_fabs(hi) : 0.0, has_lo ? __builtin_fabs(lo) : 0.0);
      const bool pre = ok && has_lo && !has_hi;
      // (FM == 2: the stored |a_r| is this very product, 0 for a zero row)
      double nrm;
      if constexpr (FM == 2) nrm = !(nrm2 <= 0.0) ? an1[r] : 0.0;
      else nrm = !(nrm2 <= 0.0) ? nrm2 * rsq1(nrm2) : 0.0;
      rg.low[r] = pre;
      rg.w[r] = (ok && has_hi && has_lo) ? hi - lo : kInf;
      bl[r] = ok ? (pre ? -lo : hi) : 0.0;
      if (pre) {
#pragma unroll
        for (int j = 0; j < NL; ++j) E[r][j] = -E[r][j];
      }
      thr[r] = !(nrm2 <= 0.0) ? -feas_tol * (nrm + beta) : -kInf;
      infeasible_row = infeasible_row ||
                       (ok && nrm2 == 0.0 &&
                        ((has_hi && hi < -feas_tol * (1.0 + __builtin_fabs(hi))) ||
                         (has_lo && lo > feas_tol * (1.0 + __builtin_fabs(lo))) ||
                         (eqr && has_hi && hi > feas_tol * (1.0 + __builtin_fabs(hi))))) ||
                       (ok && !eqr && rg.w[r] < -feas_tol * (nrm + beta));
      thr[r] = (eqr && !has_hi) ? __builtin_nan("") : thr[r];
      return;
    }
    bl[r] = ok ? (bv[r] == bv[r] ? bv[r] : kInf) : 0.0;
    if constexpr (FM == 2) thr[r] = !(nrm2 <= 0.0) ? -feas_tol * (an1[r] + __builtin_fabs(bl[r])) : -kInf;
    else thr[r] = !(nrm2 <= 0.0) ? -feas_tol * (nrm2 * rsq1(nrm2) + __builtin_fabs(bl[r])) : -kInf;
    infeasible_row = infeasible_row || (ok && nrm2 == 0.0 && bl[r] < -feas_tol * (1.0 + __builtin_fabs(bl[r])));
    if constexpr (EQ) {
      // an equality: a zero row is infeasible for b of either sign, and a
      // non-finite b cannot mean "absent" -- QPB_NUMERICAL through the NaN
      // threshold, like a NaN row
      const bool eqr = ok && l + NL * r < meq;
      infeasible_row = infeasible_row || (eqr && nrm2 == 0.0 && bl[r] > feas_tol * (1.0 + __builtin_fabs(bl[r])));
      thr[r] = (eqr && !(__builtin_fabs(bv[r]) < kInf)) ? __builtin_nan("") : thr[r];
    }
  };
  [[maybe_unused]] double fdn[MR];    // FM == 2: |D[r,:]|^2 from the buffer
  [[maybe_unused]] bool fspd = true;  // FM == 2: the buffer's H was positive definite
  if constexpr (FM == 2) {
    // The buffer in place of H and A: every load is 16 bytes per lane at
    // consecutive addresses over the QP's lanes, the same for the wave's four
    // QPs (and every other wave: the few KiB stay in the caches).  The offsets
    // depend on MR alone (qpb_factor.h).
    constexpr uint32_t oL = fct::kHdr, oD = oL + NL * NL, oN = oD + MR * NL * NL;
    static_assert(fct::layout(NL, NL * MR).L == oL && fct::layout(NL, NL * MR).D == oD &&
                  fct::layout(NL, NL * MR).an2 == oN && fct::layout(1, NL * MR).dn2 == oN + 2 * MR * NL);
    fspd = Hs[0] != (double)QPB_NOT_SPD;
    const uint32_t lo = (uint32_t)l * 16u;
#pragma unroll
    for (int t = 0; t < NL / 2; ++t) {
      const double2 v = at_off<double2>(Hs, (oL + (uint32_t)t * 2u * NL) * 8u + lo);
      Lr[2 * t] = v.x;
      Lr[2 * t + 1] = v.y;
    }
#pragma unroll
    for (int r = 0; r < MR; ++r) {
#pragma unroll
      for (int t = 0; t < NL / 2; ++t) {
        const double2 v = at_off<double2>(Hs, (oD + (uint32_t)(r * (NL / 2) + t) * 2u * NL) * 8u + lo);
        E[r][2 * t] = v.x;
        E[r][2 * t + 1] = v.y;
      }
      an2[r] = at_off<double>(Hs, (oN + (uint32_t)(r * NL)) * 8u + (uint32_t)l * 8u);
      an1[r] = at_off<double>(Hs, (oN + (uint32_t)((MR + r) * NL)) * 8u + (uint32_t)l * 8u);
      fdn[r] = at_off<double>(Hs, (oN + (uint32_t)((2 * MR + r) * NL)) * 8u + (uint32_t)l * 8u);
    }
#pragma unroll
    for (int r = 0; r < MR; ++r) row_norms(r, E[r]);
  } else if constexpr (N16) {
    // Coalesced 16-byte loads: one instruction reads 2 whole rows (256 B) of
    // each of the wave's 4 QPs -- lane l gets row 2t + (l>>3), columns
    // 2(l&7), 2(l&7)+1.  Rows reach their owner lane through a transpose in
    // this QP's LDS slot (free until the factorisation ends).
    const uint32_t hoff = (uint32_t)(hr * NL + hc) * 8u;  // row hr, column hc of a 16-column matrix
    const double *Hl = &at_off<double>(Hs, (SH ? sl * ((uint32_t)strideH * 8u) : sl * (NL * NL * 8u)) + hoff);
    const double *Al = &at_off<double>(As, (SH ? sl * ((uint32_t)strideA * 8u) : sl * umn * 8u) + hoff);
    double2 hv[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) hv[t] = *reinterpret_cast<const double2 *>(&Hl[2 * t * NL]);
    auto load_a = [&](int r, double2 (&v)[8]) {
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int row = NL * r + 2 * t + hr;
        if constexpr (BX) {
          // rows >= mg are synthesised: the lane's two columns hc, hc + 1 of
          // e_{row - mg} take the place of the loaded pair (zeros past m)
          const int jb = row < m ? row - mg : -2;
          const double2 e = make_double2(jb == hc ? 1.0 : 0.0, jb == hc + 1 ? 1.0 : 0.0);
          if constexpr (FULL)
            v[t] = r < MR - 1 ? *reinterpret_cast<const double2 *>(&Al[(NL * r + 2 * t) * NL]) : e;
          else
            v[t] = row < mg ? *reinterpret_cast<const double2 *>(&Al[(NL * r + 2 * t) * NL]) : e;
        } else if constexpr (FULL)
          v[t] = *reinterpret_cast<const double2 *>(&Al[(NL * r + 2 * t) * NL]);
        else
          v[t] = row < m ? *reinterpret_cast<const double2 *>(&Al[(NL * r + 2 * t) * NL]) : make_double2(0.0, 0.0);
      }
    };
    // all input rows in flight at once (one HBM round trip); instruction
    // selection sinks loads to their first use, so an empty asm consumes
    // them right here
    double2 av[MR][8];
#pragma unroll
    for (int r = 0; r < MR; ++r) load_a(r, av[r]);
#pragma unroll
    for (int r = 0; r < MR; ++r) asm volatile("" ::"v"(bv[r]));
    if constexpr (RG) {
#pragma unroll
      for (int r = 0; r < MR; ++r) asm volatile("" ::"v"(rg.lo[r]));
    }
    asm volatile("" ::"v"(fv));
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      asm volatile("" ::"v"(hv[t].x), "v"(hv[t].y));
#pragma unroll
      for (int r = 0; r < MR; ++r) asm volatile("" ::"v"(av[r][t].x), "v"(av[r][t].y));
    }
    stage(hv);
    lds_row16(&base[l * RS], Lr);
#pragma unroll
    for (int r = 0; r < MR; ++r) {
      stage(av[r]);
      lds_row16(&base[l * RS], E[r]);
      row_norms(r, E[r]);
    }
    wave_lds_sync();
  } else {  // padded n < 16: clamped per-lane row loads, identity outside n
    const int lc = l < n ? l : n - 1;
    const uint32_t hrow =  // the lane's row of H
        SH ? sl * (uint32_t)strideH * 8u + (uint32_t)lc * un * 8u : (sl * un + (uint32_t)lc) * un * 8u;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const double h = at_off<double>(Hs, hrow + (uint32_t)(j < n ? j : n - 1) * 8u);
      Lr[j] = (l < n && j < n) ? h : (l == j ? 1.0 : 0.0);
    }
#pragma unroll
    for (int r = 0; r < MR; ++r) {
      const int row = l + NL * r;
      const bool ok = row < m;
      const int rc = ok ? row : 0;
      const uint32_t arow_off =
          SH ? sl * (uint32_t)strideA * 8u + (uint32_t)rc * un * 8u : (sl * umn + (uint32_t)rc * un) * 8u;
      if (BX && row >= mg) {  // e_{row - mg} (zeros past m): nothing is read
#pragma unroll
        for (int j = 0; j < NL; ++j) E[r][j] = (ok && row - mg == j) ? 1.0 : 0.0;
      } else {
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          const double a = at_off<double>(As, arow_off + (uint32_t)(j < n ? j : n - 1) * 8u);
          E[r][j] = (ok && j < n) ? a : 0.0;
        }
      }
      row_norms(r, E[r]);
    }
  }
  clk.tick(0);
#ifdef QPB_WAVE_TRACE
  if (!STAMP && dbg) {  // diagnostic build: the inputs have arrived
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    if (threadIdx.x == 0) dbg[8ull * grp + 5] = t;
  }
#endif

  bool spd = true;
  double ya = fl;
  if constexpr (FM == 2) {
    // ---- y = L^{-1} f and s = b + D y from the stored L and D.  Lane-parallel
    // forward substitution on the negated accumulator na = -(f - sum L y): step k
    // forms t = na ninv, which is y_k on lane k (ninv = -1 / L[l][l]), and every
    // FMA of the step reads it from lane k by its own DPP broadcast -- the MR
    // rows' s += D[r][k] y_k and the lane's na += L[l][k] y_k.  t is a VALU
    // result read through DPP: dpp_ready issues the wait states.  Lane k's own na
    // becomes 0 at step k and is dead from there on, like the entries of its row
    // of L right of the diagonal (zero in the buffer).
    spd = fspd;
    store_l(Lp, l, Lr);  // kept for the final solves
    const double ninv = -rcp1(Lp[lrow(l) + l]);
    wave_lds_sync();
    double na = -ya;
#pragma unroll
    for (int r = 0; r < MR; ++r) s[r] = bl[r];
    unroll<NL>([&](auto K) {
      constexpr int k = K;
      const double t = na * ninv;
      dpp_ready(t);
#pragma unroll
      for (int r = 0; r < MR; ++r) fmac_bc<k>(s[r], t, E[r][k]);
      fmac_bc<k>(na, t, Lr[k]);
    });
  } else {
    // ---- H = L L^T, D = A L^{-T}, y = L^{-1} f: one right-looking sweep.
    // Step k: pr = row k of the current Schur complement (lane k's Lr, DPP
    // broadcast) = column k by symmetry, so L[j][k] = pr[j] / sqrt(akk) and
    //   row l:  Lr[j] -= c pr[j] (j > k),  c = Lr[k] / akk;   Lr[k] = L[l][k]
    //   D rows: E[k] /= sqrt(akk), E[j] -= E[k] pr[j] / akk (j > k)
    //   y:      lane-parallel, f_l -= c f_k (f_k read from lane k by the FMA)
    // Lanes l < k keep updating dead entries of their row (the upper triangle,
    // never read).  The pivot row is read straight from lane k by the FMAs
    // (v_fmac_f64_dpp); the sched_barrier and the rsq chain keep every write of
    // Lr[j] and of f (previous step) well over two instructions before these
    // reads.  Lane k's own Lr[j] is updated last, after the D rows have read it.
    // s = b + D y accumulates in the same sweep, negated: D[r][k] y_k =
    // (e ik)(f_k ik) = -ne2 f_k, one DPP-fused FMA per row with f_k from lane k
    // (y itself is never formed).
    double ns[MR];  // -s during the sweep
#pragma unroll
    for (int r = 0; r < MR; ++r) ns[r] = -bl[r];
    unroll<NL>([&](auto K) {
      constexpr int k = K;
      __builtin_amdgcn_sched_barrier(0);
      const double akk = bc<k>(Lr[k]);
      spd = spd && (akk > 0.0);
      const double ik = rsq1(akk);
      const double ik2 = ik * ik;
      const double nc = -(Lr[k] * ik2);
      double ne2[MR];
#pragma unroll
      for (int r = 0; r < MR; ++r) {
        const double e = E[r][k];
        ne2[r] = -(e * ik2);
        E[r][k] = e * ik;
      }
#pragma unroll
      for (int r = 0; r < MR; ++r) fmac_bc<k>(ns[r], ya, ne2[r]);
      unroll<NL - 1 - k>([&](auto J) {
        constexpr int j = k + 1 + J;
#pragma unroll
        for (int r = 0; r < MR; ++r) fmac_bc<k>(E[r][j], Lr[j], ne2[r]);
        fmac_bc<k>(Lr[j], Lr[j], nc);
      });
      fmac_bc<k>(ya, ya, nc);  // lane k's own f_k becomes 0 (dead)
      Lr[k] *= ik;
    });
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < MR; ++r) s[r] = -ns[r];
    store_l(Lp, l, Lr);  // kept for the final solves
  }
  // |D[r,:]|^2 = |a_r L^{-T}|^2: the loop's reflections are orthogonal, so it
  // never changes (the dependency test's scale).  Clamped to FLT_MAX instead
  // of overflowing to inf (rows with |D_r| > 1.8e19, e.g. |a| = 1e20 over a
  // unit H): the test |d2|^2 > 1e-24 |D_p|^2 then still rejects a dependent
  // row (|d2|^2 ~ eps^2 |D_p|^2) up to |D_p| ~ 1e23, where it used to reject
  // every row and end the QP INFEASIBLE.
#pragma unroll
  for (int r = 0; r < MR; ++r) {
    if constexpr (FM == 2)
      ddr[r] = (float)fdn[r];
    else
      ddr[r] = __builtin_fminf((float)dot2<NL>([&](int j) { return E[r][j]; }, [&](int j) { return E[r][j]; }),
                               3.402823466e38f);
    fn2[r] = ddr[r];
  }
  if constexpr (FM == 1) {
    // ---- the factor kernel ends here: the live row (QP 0) writes the buffer
    bool nan_row = false;
#pragma unroll
    for (int r = 0; r < MR; ++r) nan_row = nan_row || ((FULL || l + NL * r < m) && !(an2[r] < kInf));
    const bool anynan = row_min(nan_row ? -1.0 : 0.0) < 0.0;
    const int found = !spd ? QPB_NOT_SPD : anynan ? QPB_NUMERICAL : QPB_OK;
    if (live) {
      constexpr int oL = fct::kHdr, oD = oL + NL * NL, oN = oD + MR * NL * NL, oA = oN + 3 * MR * NL;
      static_assert(fct::layout(NL, NL * MR).D == oD && fct::layout(NL, NL * MR).an2 == oN &&
                    fct::layout(1, NL * MR).A == oA && fct::layout(NL, NL * MR).size == oA + NL * NL * MR);
      double *fac = xg;
      if (l < fct::kHdr) fac[l] = l == 0 ? (double)found : l == 1 ? (double)n : l == 2 ? (double)m : l == 3 ? 16.0 : 0.0;
      if (l == 0 && statg) statg[0] = found;
#pragma unroll
      for (int t = 0; t < NL / 2; ++t)  // zero right of the diagonal (the sweep leaves dead values there)
        *reinterpret_cast<double2 *>(&fac[oL + (t * NL + l) * 2]) =
            make_double2(2 * t <= l ? Lr[2 * t] : 0.0, 2 * t + 1 <= l ? Lr[2 * t + 1] : 0.0);
#pragma unroll
      for (int r = 0; r < MR; ++r) {
#pragma unroll
        for (int t = 0; t < NL / 2; ++t)
          *reinterpret_cast<double2 *>(&fac[oD + ((r * (NL / 2) + t) * NL + l) * 2]) =
              make_double2(E[r][2 * t], E[r][2 * t + 1]);
        fac[oN + r * NL + l] = an2[r];
        fac[oN + (MR + r) * NL + l] = an1[r];
        fac[oN + (2 * MR + r) * NL + l] = (double)ddr[r];
      }
      for (int i = l; i < m * n; i += NL) fac[oA + i] = As[i];
    }
    return;
  }
  clk.tick(1);

  // ------------------------------------------------------ active-set loop
  // R (upper triangular, active positions; column j = position j, column-major
  // so the lane-parallel accesses are contiguous) lives in LDS with a ZERO
  // diagonal; lane l keeps 1 / R[l][l] in a register, so the back
  // substitution needs no masking.
#pragma unroll
  for (int j = 0; j < NL; j += 2) *reinterpret_cast<double2 *>(&Tv[l * NL + j]) = make_double2(0.0, 0.0);
  int q = 0;           // active-set size
  double um = 0.0;     // multiplier of active position l
  int iam = -1;        // constraint index at active position l
  double invRd = 0.0;  // 1 / R[l][l]
  int status;
  bool done;
  {
    // any lane seeing an infeasible zero row (-1) or a NaN row (-2) marks the
    // whole QP
    bool nan_row = false;
#pragma unroll
    for (int r = 0; r < MR; ++r) nan_row = nan_row || thr[r] != thr[r];
    // (a NaN here is an input's; a QP that has one never enters the loop, where
    // a NaN high word comes to mean "active")
#pragma unroll
    for (int r = 0; r < MR; ++r) thh[r] = hi32(thr[r]);
    const double bad = row_min(nan_row ? -2.0 : infeasible_row ? -1.0 : 0.0);
    const bool inf0 = bad < 0.0;
    status = !spd ? QPB_NOT_SPD : (bad < -1.5 ? QPB_NUMERICAL : inf0 ? QPB_INFEASIBLE : QPB_MAX_ITER);
    done = !spd || inf0;
  }
  bool selecting = true;
  int p = 0;
  double up = 0.0;  // multiplier of the constraint being added
  int it = 0;
  [[maybe_unused]] EqState<EQ> eqs;
  wave_lds_sync();
  clk.tick(3);

  while (!done && it < max_iter) {
    ++it;
    if constexpr (RG) rg.fresh = false;
    if constexpr (EQ) {
      // the equality phase: one row per trip, whatever its slack (it ends in
      // an ADD or leaves the row out, never in a partial step)
      eqs.sel = selecting && eqs.next < meq;
      if (eqs.sel) {
        p = eqs.next++;
        up = 0.0;
        selecting = false;
      }
    }
    if (selecting) {
      // The violation test is fp64 on the slack normalised by |a_row| (the
      // feasibility tolerance); among the violated rows the argmax runs on
      // 32-bit keys: the fp32 violation per unit length of the row's free
      // part, -s / |D[r, q:]| (dual steepest edge: 4.66 instead of 5.05
      // iterations per QP on the bench family, 6.18 instead of 6.97 on the
      // dense one, tools/gi_select_sim.py), row index in the low 5 bits, so
      // one DPP-fused v_max_u32 per step reduces the row (0 = none violated)
      uint32_t key = 0u;
#pragma unroll
      for (int r = 0; r < MR; ++r) {
        if constexpr (RG) {
          // the more violated side of the row: the one held (s) or the other
          // (w - s; NaN or +inf where the row has no other side), same key
          const double so = rg.w[r] - s[r];
          const double sv = so < s[r] ? so : s[r];
          const bool viol = sv < thr[r];  // false for an active row (thr NaN)
          const float kf = __builtin_fmaf((float)(-sv), __builtin_amdgcn_rsqf(fn2[r]), 0x1p-100f);
          const uint32_t kr = (__float_as_uint(kf) & ~31u) | (uint32_t)(l + NL * r);
          key = viol && kr > key && l + NL * r >= meq ? kr : key;
          continue;
        }
        const bool viol = s[r] < thr[r];  // false for an active row (thr NaN)
        // fn2 in [0, FLT_MAX] (clamped where it shrinks); the 2^-100 floor keeps
        // a violated row's key above 31 -- never 0, the "none violated" key --
        // when the ratio underflows (row 0 included)
        const float kf = __builtin_fmaf((float)(-s[r]), __builtin_amdgcn_rsqf(fn2[r]), 0x1p-100f);
        const uint32_t kr = (__float_as_uint(kf) & ~31u) | (uint32_t)(l + NL * r);
        if constexpr (EQ)  // the equalities had their turn
          key = viol && kr > key && l + NL * r >= meq ? kr : key;
        else
          key = viol && kr > key ? kr : key;
      }
      key = row_max_u32(key);
      if (key == 0u) {
        status = QPB_OK;
        done = true;
        break;
      }
      p = (int)(key & 31u);
      up = 0.0;
      selecting = false;
      if constexpr (RG) rg.fresh = true;
    }
    clk.tick(4);
    // wave-uniform bound on the active set size (q <= NL always; the clamp
    // keeps every R column loop inside the QP's slot regardless)
    const int qmax = __builtin_elementwise_min(wave_max4(q), NL);

    // ---- row p of D, s_p and |D[p,:]|^2 through the exchange row; lane l
    // keeps its entry D[p][l] (d = -D[p,:] in G-I's sign convention; the
    // signs are folded into the formulas below)
    const int owner = p & (NL - 1), prow = p >> 4;
    if constexpr (EQ) {
      // an equality met on its a x < b side becomes -a x <= -b: row p of D and
      // s_p change sign in place, and the QP's lanes learn of it
      if (eqs.sel) {
        uint32_t neg = 0u;
        if (l == owner) {
#pragma unroll
          for (int r = 0; r < MR; ++r)
            if (r == prow && s[r] > 0.0) {
#pragma unroll
              for (int j = 0; j < NL; ++j) E[r][j] = -E[r][j];
              s[r] = -s[r];
              neg = 1u;
              if constexpr (RG) rg.low[r] = !rg.low[r];
            }
        }
        eqs.flip = row_max_u32(neg) != 0u;
      }
    }
    if constexpr (RG) {
      // a row just selected on the side it is not held on changes sides: row p
      // of D negated in place, s_p = w - s_p; then the QP's lanes learn which
      // side row p is on (an equality's flip above included)
      uint32_t lw = 0u;
      if (l == owner) {
#pragma unroll
        for (int r = 0; r < MR; ++r)
          if (r == prow) {
            if (rg.fresh && rg.w[r] - s[r] < s[r]) {
#pragma unroll
              for (int j = 0; j < NL; ++j) E[r][j] = -E[r][j];
              s[r] = rg.w[r] - s[r];
              rg.low[r] = !rg.low[r];
            }
            lw = rg.low[r] ? 1u : 0u;
          }
      }
      rg.plow = row_max_u32(lw) != 0u;
    }
    if (l == owner) {
#pragma unroll
      for (int r = 0; r < MR; ++r)
        if (r == prow) {
#pragma unroll
          for (int j = 0; j < NL; j += 2) *reinterpret_cast<double2 *>(&xch[j]) = make_double2(E[r][j], E[r][j + 1]);
          *reinterpret_cast<double2 *>(xsd) = make_double2(s[r], (double)ddr[r]);
        }
    }
    wave_lds_sync();
    const double Dpl = xch[l];
    const double2 spdd = *reinterpret_cast<const double2 *>(xsd);
    const double Dpq = xch[q & (NL - 1)];  // q == 16: an ADD is impossible (d2 = 0)
    const double sp = spdd.x, dd = spdd.y;  // s_p, |D[p,:]|^2
    wave_lds_sync();
    const double d2 = (l >= q) ? Dpl : 0.0;  // D[p, q:]
    dpp_ready(d2);
    // slack direction D d2 (d2 read from lane j by the FMAs)
    double u[MR];
    bdot_rows<MR>(d2, E, u);
    const double nd2 = row_sum(d2 * d2);  // |d2|^2
    clk.tick(5);

    // ---- r = R^{-1} d1: lane-parallel back substitution over the active positions
    double rm = 0.0;
    if (qmax > 0) {
      // on the negated accumulator (back_subst_step)
      const double ninv = -invRd;
      double nacc = (l < q) ? Dpl : 0.0;  // = -d1_l
      // steps 15 .. 1 in that order (column 0 holds no entry above the
      // diagonal: skipped), each behind its wave-uniform test j < qmax.  The
      // tests are grouped 15..8, 7..4, 3..1 under one test per group: a flat
      // chain walked 12 to 14 failing tests per trip at the usual qmax of 2 or
      // 3 (one scalar compare and branch each), the groups walk 1 + 3.
      auto step = [&](auto JC) { back_subst_step<JC>(Tv, l, qmax, nacc, ninv); };
      if (qmax > 4) {
        if (qmax > 8) unroll<8>([&](auto JJ) { step(std::integral_constant<int, NL - 1 - JJ>{}); });
        unroll<4>([&](auto JJ) { step(std::integral_constant<int, 7 - JJ>{}); });
      }
      unroll<3>([&](auto JJ) { step(std::integral_constant<int, 3 - JJ>{}); });
      rm = nacc * ninv;  // r_l (0 for l >= q)
    }
    clk.tick(6);

    // ---- step lengths
    double t1 = kBig;
    bool attains = false;  // this position attains the minimum ratio (read by a DROP only)
    if (qmax > 0) {
      // the exact minimum ratio; a DROP then takes the lowest position attaining it
      const double ratio = um * rcp1(rm);
      const bool cand = l < q && rm > 0.0;
      if constexpr (EQ) {  // an equality is never dropped
        const bool cdrop = cand && l >= eqs.q;
        t1 = row_min_raw(cdrop ? ratio : kBig);
        attains = cdrop && ratio == t1;
      } else {
        t1 = row_min_raw(cand ? ratio : kBig);
        attains = cand && ratio == t1;
      }
    }
    const double ir = rsq1(nd2);  // 1/|d2| (only used when nd2 > 0)
    const double t2 = (nd2 > kDepTol * dd) ? -sp * (ir * ir) : kBig;
    const double t = t1 < t2 ? t1 : t2;
    if (!(t < kBig)) {
      if constexpr (EQ) {
        // an equality that depends on those before it (or a zero row, or any
        // row once q = n): its residual |a x - b| can no longer change; within
        // the tolerance the row is left out and the solve goes on
        if (eqs.sel) {
          uint32_t within = 0u;
#pragma unroll
          for (int r = 0; r < MR; ++r)
            within |= (l == owner && r == prow && __builtin_fabs(s[r]) <= -thr[r]) ? 1u : 0u;
          if (row_max_u32(within) != 0u) {
            selecting = true;
            wave_lds_sync();
            continue;
          }
        }
      }
      status = QPB_INFEASIBLE;
      done = true;
      break;
    }
    if (t2 < kBig) {  // primal step: slacks s -= t A z,  A z = -D[:, q:] d2
#pragma unroll
      for (int r = 0; r < MR; ++r) s[r] = __builtin_fma(t, u[r], s[r]);
    }
    um = __builtin_fma(-t, rm, um);
    up += t;
    clk.tick(7);

    if (t2 <= t1) {
      // ---------------- ADD p: Householder on columns q.. of D.  With
      // dq = -D[p,q]: alpha = -sign(dq) |d2|, v = d2 + alpha e_q (the negated
      // G-I vector: same reflection), beta = 1 / (|d2|^2 + alpha D[p,q]) =
      // 1 / (|d2| (|d2| + |D[p,q]|)): one reciprocal.
      const double nrm = nd2 * ir;
      const bool neg = Dpq <= 0.0;
      const double alpha = neg ? -nrm : nrm;
      const double beta = ir * rcp1(nrm + __builtin_fabs(Dpq));
      const double ia = neg ? -ir : ir;  // 1 / alpha
      const double v = d2 + (l == q ? alpha : 0.0);
      // E v = E d2 + alpha E[:, q] = u + alpha E[:, q]: no second product;
      // column q by a branch tree on q (its distinct values in the wave)
      double nw[MR];
      switch (q & (NL - 1)) {
#define QPB_COLQ_CASE(J)                                        \
  case J:                                                        \
    asm volatile("");                                            \
    for (int r = 0; r < MR; ++r) nw[r] = E[r][J];                \
    break;
        QPB_COLQ_CASE(0) QPB_COLQ_CASE(1) QPB_COLQ_CASE(2) QPB_COLQ_CASE(3)
        QPB_COLQ_CASE(4) QPB_COLQ_CASE(5) QPB_COLQ_CASE(6) QPB_COLQ_CASE(7)
        QPB_COLQ_CASE(8) QPB_COLQ_CASE(9) QPB_COLQ_CASE(10) QPB_COLQ_CASE(11)
        QPB_COLQ_CASE(12) QPB_COLQ_CASE(13) QPB_COLQ_CASE(14) QPB_COLQ_CASE(15)
#undef QPB_COLQ_CASE
      }
#pragma unroll
      for (int r = 0; r < MR; ++r) nw[r] = -beta * __builtin_fma(alpha, nw[r], u[r]);
      dpp_ready(v);
#pragma unroll
      for (int r = 0; r < MR; ++r) unroll<NL>([&](auto J) {
          constexpr int j = J;
          fmac_bc<j>(E[r][j], v, nw[r]);
        });
      // the reflection maps e_q to -d2 / alpha: column q of the new D is
      // -u / alpha, and it leaves the free part of every row
#pragma unroll
      for (int r = 0; r < MR; ++r) {
        const float c = (float)(u[r] * ia);
        fn2[r] = __builtin_fmaxf(__builtin_fmaf(-c, c, fn2[r]), 0.0f);
      }
      // new column q of R: d1 strictly above the diagonal, alpha on it
      Tv[q * NL + l] = (l < q) ? -Dpl : 0.0;
      if (l == q) {
        invRd = ia;
        iam = p;
        um = up;
        if constexpr (RG) eqs.pneg = rg.plow;
        else if constexpr (EQ) eqs.pneg = eqs.sel && eqs.flip;
      }
#pragma unroll
      for (int r = 0; r < MR; ++r) thr[r] = with_hi32(thr[r], (l == owner && r == prow) ? kActiveHi : hi32(thr[r]));
      if constexpr (EQ) eqs.q += eqs.sel ? 1 : 0;
      ++q;
      selecting = true;
      clk.tick(8);
    } else {
      // ---------------- DROP active position k, the lowest one attaining t1
      // (the argmin is paid here, not on every trip: ADDs never read it)
      const int k = (int)row_min_u32(attains ? (uint32_t)l : 31u) & (NL - 1);
      const int c = __shfl(iam, k, NL);
#pragma unroll
      for (int r = 0; r < MR; ++r)
        thr[r] = with_hi32(thr[r], (l == (c & (NL - 1)) && r == (c >> 4)) ? thh[r] : hi32(thr[r]));
      const double un = __shfl(um, (l + 1) & (NL - 1), NL);
      const int in = __shfl(iam, (l + 1) & (NL - 1), NL);
      if (l >= k && l < q - 1) {
        um = un;
        iam = in;
      } else if (l == q - 1) {
        um = 0.0;
        iam = -1;
      }
      if constexpr (RG) {  // the position's side moves with um and iam
        const bool pn = __shfl((int)eqs.pneg, (l + 1) & (NL - 1), NL) != 0;
        eqs.pneg = (l >= k && l < q - 1) ? pn : (l == q - 1 ? false : eqs.pneg);
      }
      // full R (diagonal put back), delete column k: lane l (column l) reads
      // column l + 1 whole, then writes it (in-order DS: every read precedes
      // every write)
      wave_lds_sync();
      if (l < q) Tv[l * NL + l] = rcp1(invRd);  // R[l][l] (alpha when it was added)
      wave_lds_sync();
      {
        double col[NL];
        lds_row16(&Tv[((l + 1) & (NL - 1)) * NL], col);
        wave_lds_sync();
        if (l >= k && l < q - 1) {
#pragma unroll
          for (int j = 0; j < NL; j += 2) *reinterpret_cast<double2 *>(&Tv[l * NL + j]) = make_double2(col[j], col[j + 1]);
        } else if (l == q - 1) {
#pragma unroll
          for (int j = 0; j < NL; j += 2) *reinterpret_cast<double2 *>(&Tv[l * NL + j]) = make_double2(0.0, 0.0);
        }
      }
      // Givens rotations restore the upper-triangular R; lane j keeps the
      // parameters of rotation j, which the unrolled D update reads by DPP
      double gc = 0.0, gs = 0.0;
      for (int j = k; j < q - 1; ++j) {
        wave_lds_sync();
        const double a = Tv[j * NL + j], bb = Tv[j * NL + j + 1];
        const double irr = rsq1(__builtin_fma(a, a, bb * bb));
        const double cj = a * irr, sj = bb * irr;
        const double rj = Tv[l * NL + j], rj1 = Tv[l * NL + j + 1];
        wave_lds_sync();
        if (l >= j && l < q - 1) {
          Tv[l * NL + j] = __builtin_fma(cj, rj, sj * rj1);
          Tv[l * NL + j + 1] = (l == j) ? 0.0 : __builtin_fma(-sj, rj, cj * rj1);
        }
        if (l == j) {
          gc = cj;
          gs = sj;
        }
      }
      wave_lds_sync();
      Tv[l * NL + q - 1] = 0.0;
      unroll<NL - 1>([&](auto JJ) {
        constexpr int j = JJ;
        if (j + 1 < qmax && j >= k && j < q - 1) {
          const double cj = bc<j>(gc), sj = bc<j>(gs);
#pragma unroll
          for (int r = 0; r < MR; ++r) rotate_pair<j>(E[r], cj, sj);
        }
      });
      --q;
      // column q (after the rotations) joins the free part: recompute
#pragma unroll
      for (int r = 0; r < MR; ++r) {
        float a0 = 0.0f, a1 = 0.0f;
        unroll<NL>([&](auto J) {
          constexpr int j = J;
          const float e = (float)E[r][j];
          if constexpr (j % 2 == 0) a0 = __builtin_fmaf(e, j >= q ? e : 0.0f, a0);
          if constexpr (j % 2 == 1) a1 = __builtin_fmaf(e, j >= q ? e : 0.0f, a1);
        });
        fn2[r] = a0 + a1;
      }
      const double dg = take_diagonal(Tv, l, q);
      invRd = (l < q) ? rcp1(dg) : 0.0;
      clk.tick(9);
    }
    wave_lds_sync();
  }
  clk.tick(10);
#ifdef QPB_WAVE_TRACE
  if (!STAMP) wave_stamp32(dbg, grp, 12);  // the loop has ended
#endif
  // EQ: from here on the multiplier of the caller's row (a flipped equality's is -um)
  // RG: the clamp first, on the multiplier of the side held; then the sign of
  // a lower-side position, so that H x + f + A^T lam = 0 with the caller's A
  if constexpr (RG) {
    um = l >= eqs.q ? dual_out(um) : um;
    um = eqs.pneg ? -um : um;
  } else {
    if constexpr (EQ) um = eqs.pneg ? -um : um;
    // lam >= 0 on the inequalities' positions (dual_out: a tie's -eps written as 0)
    if constexpr (EQ) um = l >= eqs.q ? dual_out(um) : um;
    else um = dual_out(um);
  }

  // ------------------------------------------------------------- outputs
  // (the active rows of A re-read, one coalesced 128-B row per active position)
  const int qm = __builtin_elementwise_min(wave_max4(q), NL);
  // The group's scalar bases and the lane's QP inside the group again,
  // recomputed from opaque copies of the group index and the slot instead of
  // held across the loop (held, the allocator spilled them)
  int slot_o = slot;
  asm volatile("" : "+v"(slot_o));
  long long grp_o = grp;
  asm volatile("" : "+s"(grp_o));
  const long long go0 = grp_o * QPB;
  const int rem_o = (int)__builtin_elementwise_min(batch - go0, (long long)QPB);
  const bool live_o = slot_o < rem_o;
  const uint32_t slo = (uint32_t)(live_o ? slot_o : rem_o - 1);
  const long long gio0 =
      (flags & QPB_FLAG_DIAG_L2) ? (go0 & 511) : (flags & QPB_FLAG_DIAG_MALL) ? (go0 & 16383) : go0;
  const double *Aso = SH ? ((BX ? mg : m) > 0 ? Ag + gio0 * strideA : Hg + gio0 * strideH)
                         : (m > 0 ? Ag + gio0 * (long long)m * n : Hg + gio0 * (long long)n * n);
  // The A-row loads go out first, in at most two groups of eight (one
  // wave-uniform test per group: a test per load made each load a branch
  // with its own wait); the work that does not need them -- the multipliers by
  // row and their stores, the active-set word, L's row -- runs while they are
  // in flight.  Positions past qm read a valid row and are not summed.
  // Addresses: the byte offset of the position's row (m <= 32 rows of n <= 16
  // doubles: below 4 KiB) is formed once per lane, before the broadcast, and
  // each load adds the broadcast offset to this lane's 32-bit column offset
  // inside the group's A block -- a DPP move and one 32-bit add per load on the
  // group's scalar base.
  // BX: a position whose row is mg + j holds a variable's bound and adds
  // um e_j: jbx is j there and -1 elsewhere, nothing of G is needed for it (its
  // load goes to row 0, the line the others' loads have brought in, and its
  // value is not used), and with mg == 0 no load goes out at all
  const uint32_t iob = (uint32_t)((iam > 0 && (!BX || iam < mg)) ? iam : 0) * (uint32_t)n * 8u;
  asm volatile("s_nop 1" ::"v"(iob));  // its DPP reads below may sit behind a branch only
  [[maybe_unused]] const int jbx = (BX && iam >= mg) ? iam - mg : -1;
  if constexpr (BX) asm volatile("s_nop 1" ::"v"(jbx));
  const int lc = l < n ? l : n - 1;
  const uint32_t acol = SH ? slo * ((uint32_t)strideA * 8u) + (uint32_t)lc * 8u
                           : (slo * (uint32_t)m * (uint32_t)n + (uint32_t)lc) * 8u;
  double arow[NL];
  if constexpr (BX) {
#pragma unroll
    for (int k = 0; k < NL; ++k) arow[k] = 0.0;
  }
  unroll<2>([&](auto H) {
    constexpr int k0 = 8 * H;
    if (k0 < qm && (!BX || mg > 0)) {
      __builtin_amdgcn_sched_barrier(0);
      unroll<8>([&](auto K) {
        constexpr int kk = k0 + K;
        arow[kk] = at_off<double>(Aso, acol + (uint32_t)bci<kk>((int)iob));
      });
    }
  });
  double *lamb = Tv;  // lambda scatter (32) over the dead R
#pragma unroll
  for (int r = 0; r < 2; ++r) lamb[l + NL * r] = 0.0;
  wave_lds_sync();
  if (l < q && iam >= 0) lamb[iam] = um;
  wave_lds_sync();
  double lamr[MR];
#pragma unroll
  for (int r = 0; r < MR; ++r) lamr[r] = lamb[l + NL * r];
  const double invd = rcp1(Lp[lrow(l) + l]);
  double Lrow[NL];  // row l of L (entries past l are dead)
#pragma unroll
  for (int j = 0; j < NL; ++j) Lrow[j] = Lp[lrow(l) + j];
  wave_lds_sync();
#pragma unroll
  for (int r = 0; r < MR; ++r) {
    const int row = l + NL * r;
    if (live_o && (FULL || row < m))
      at_off<double>(lamg + go0 * m, (slo * (uint32_t)m + (uint32_t)row) * 8u) = lamr[r];
  }
  // row r of the lane is in the active set: its threshold carries the NaN word.
  // A QP that ran no trip has no active row -- it may hold an input's NaN.
  auto in_set = [&](int r) { return it != 0 && thr[r] != thr[r]; };
  uint32_t w0 = 0;
#pragma unroll
  for (int r = 0; r < MR; ++r) {
    const unsigned long long bal = __ballot(in_set(r));
    w0 |= (uint32_t)((bal >> sh) & 0xFFFFull) << (16 * r);
  }
  if (live_o && l == 0 && m > 0) at_off<uint32_t>(actg + go0, slo * 4u) = w0;
  if constexpr (RG) {  // the rows active at their lower bound (never an equality)
    uint32_t w1 = 0;
#pragma unroll
    for (int r = 0; r < MR; ++r) {
      const unsigned long long bal = __ballot(in_set(r) && rg.low[r] && l + NL * r >= meq);
      w1 |= (uint32_t)((bal >> sh) & 0xFFFFull) << (16 * r);
    }
    if (lowg && live_o && l == 0 && m > 0) at_off<uint32_t>(lowg + go0, slo * 4u) = w1;
  }
  // x = -H^{-1} (f + A^T lam): g = f + sum_k u_k a_{iam_k}, then the two solves
  double gl = fl;
#ifdef QPB_WAVE_TRACE
  if (!STAMP) {
    // before and after the wait for the gathered rows: the empty asm reads
    // every row asked for, so the compiler's own wait stands in front of it
    wave_stamp32(dbg, grp, 13);
    unroll<2>([&](auto H) {
      constexpr int k0 = 8 * H;
      if (k0 < qm) {
        unroll<8>([&](auto K) {
          constexpr int kk = k0 + K;
          const double arrived = arow[kk];
          asm volatile("" ::"v"(arrived));
        });
      }
    });
    wave_stamp32(dbg, grp, 14);  // the gather has arrived
  }
#endif
  unroll<2>([&](auto H) {
    constexpr int k0 = 8 * H;
    if (k0 < qm) {
      unroll<8>([&](auto K) {
        constexpr int kk = k0 + K;
        if constexpr (BX) {
          // the fused multiply-add the materialised form does on the unit row's entry
          const int jb = bci<kk>(jbx);
          const double a = jb < 0 ? ((N16 || l < n) ? arow[kk] : 0.0) : (l == jb ? 1.0 : 0.0);
          if (kk < qm) gl = __builtin_fma(bc<kk>(um), a, gl);
        } else {
          if (kk < qm) gl = __builtin_fma(bc<kk>(um), (N16 || l < n) ? arow[kk] : 0.0, gl);
        }
      });
    }
  });
  const double xl = solve_x_frozen(gl, invd, Lrow, Lp, l);
#ifdef QPB_WAVE_TRACE
  if (!STAMP) {
    asm volatile("" ::"v"(xl));
    wave_stamp32(dbg, grp, 15);  // x is solved
  }
#endif
  status = x_status(status, xl);
  if (live_o && (N16 || l < n)) at_off<double>(xg + go0 * n, (slo * (uint32_t)n + (uint32_t)l) * 8u) = xl;
  if (live_o && l == 0) {
    at_off<int32_t>(statg + go0, slo * 4u) = status;
    if (itg) at_off<int32_t>(itg + go0, slo * 4u) = it;
  }
  clk.tick(11);
  clk.flush(dbg);
}

template <int MR, bool N16, bool FULL, bool STAMP = false, int OCC = 2>
__global__ __launch_bounds__(64, OCC) void gi_dense_kernel(
    const double *__restrict__ Hg, const double *__restrict__ fg, const double *__restrict__ Ag,
    const double *__restrict__ bg, double *__restrict__ xg, double *__restrict__ lamg,
    uint32_t *__restrict__ actg, int32_t *__restrict__ statg, int32_t *__restrict__ itg, int n, int m,
    long long batch, int max_iter, double feas_tol, int flags = 0,
    unsigned long long *__restrict__ dbg = nullptr) {
  __shared__ double lds[QPB * SLOT];
#ifdef QPB_WAVE_TRACE
  // diagnostic build only (tools/wave_timeline.py): each wave's start and end
  // on the 100 MHz real-time and the shader clocks, and where it ran
  unsigned long long rt0, mt0, rt1, mt1;
  unsigned hw, xcc;
  asm volatile("s_memrealtime %0\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt0), "=s"(mt0)::"memory");
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
#endif
  gi_group<MR, N16, FULL, STAMP>(lds, Hg, fg, Ag, bg, xg, lamg, actg, statg, itg, n, m, batch, max_iter, feas_tol,
#ifdef QPB_WAVE_TRACE
                                 flags, dbg, blockIdx.x);
#else
                                 flags, STAMP ? dbg : nullptr, blockIdx.x);
#endif
#ifdef QPB_WAVE_TRACE
#if QPB_WAVE_TRACE == 2
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the end after the output stores have drained
#endif
  asm volatile("s_memrealtime %0\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt1), "=s"(mt1)::"memory");
  if (!STAMP && dbg && threadIdx.x == 0) {
    unsigned long long *r = dbg + 8ull * blockIdx.x;
    r[0] = rt0;
    r[1] = rt1;
    r[2] = mt0;
    r[3] = mt1;
    r[4] = hw | ((unsigned long long)xcc << 32);
  }
#endif
}

// qpb_solve_eq's form of the kernel: gi_group with EQ, rows 0 .. meq-1 equalities
constexpr int kEqOcc = 3;  // waves per SIMD the EQ forms are built for
template <int MR, bool N16, bool FULL, int OCC>
__global__ __launch_bounds__(64, OCC) void gi_dense_eq_kernel(
    const double *__restrict__ Hg, const double *__restrict__ fg, const double *__restrict__ Ag,
    const double *__restrict__ bg, double *__restrict__ xg, double *__restrict__ lamg,
    uint32_t *__restrict__ actg, int32_t *__restrict__ statg, int32_t *__restrict__ itg, int n, int m, int meq,
    long long batch, int max_iter, double feas_tol) {
  __shared__ double lds[QPB * SLOT];
  gi_group<MR, N16, FULL, false, true>(lds, Hg, fg, Ag, bg, xg, lamg, actg, statg, itg, n, m, batch, max_iter,
                                       feas_tol, 0, nullptr, blockIdx.x, meq);
}

// qpb_solve_shared's form: gi_group with SH, with or without equality rows
template <int MR, bool N16, bool FULL, bool EQ, int OCC>
__global__ __launch_bounds__(64, OCC) void gi_dense_shared_kernel(
    const double *__restrict__ Hg, const double *__restrict__ fg, const double *__restrict__ Ag,
    const double *__restrict__ bg, double *__restrict__ xg, double *__restrict__ lamg,
    uint32_t *__restrict__ actg, int32_t *__restrict__ statg, int32_t *__restrict__ itg, int n, int m, int meq,
    long long batch, int max_iter, double feas_tol, long long strideH, long long strideA) {
  __shared__ double lds[QPB * SLOT];
  gi_group<MR, N16, FULL, false, EQ, true>(lds, Hg, fg, Ag, bg, xg, lamg, actg, statg, itg, n, m, batch, max_iter,
                                           feas_tol, 0, nullptr, blockIdx.x, meq, strideH, strideA);
}

// qpb_solve_range's form: gi_group with RG (on EQ and SH: meq and the strides
// are arguments, so one set of forms serves plain, equality and shared calls)
template <int MR, bool N16, bool FULL, int OCC>
__global__ __launch_bounds__(64, OCC) void gi_dense_range_kernel(
    const double *__restrict__ Hg, const double *__restrict__ fg, const double *__restrict__ Ag,
    const double *__restrict__ blg, const double *__restrict__ bug, double *__restrict__ xg,
    double *__restrict__ lamg, uint32_t *__restrict__ actg, uint32_t *__restrict__ lowg,
    int32_t *__restrict__ statg, int32_t *__restrict__ itg, int n, int m, int meq, long long batch, int max_iter,
    double feas_tol, long long strideH, long long strideA) {
  __shared__ double lds[QPB * SLOT];
  gi_group<MR, N16, FULL, false, true, true, true>(lds, Hg, fg, Ag, bug, xg, lamg, actg, statg, itg, n, m, batch,
                                                   max_iter, feas_tol, 0, nullptr, blockIdx.x, meq, strideH, strideA,
                                                   blg, lowg);
}

// qpb_solve_range_box's form: the range form with BX.  `m` counts all rows,
// mg + n; rows mg .. m-1 are the variables' bounds lbg <= x <= ubg (n per QP,
// either may be NULL), whose rows of A -- the identity -- are synthesised
template <int MR, bool N16, bool FULL, int OCC>
__global__ __launch_bounds__(64, OCC) void gi_dense_range_box_kernel(
    const double *__restrict__ Hg, const double *__restrict__ fg, const double *__restrict__ Gg,
    const double *__restrict__ blg, const double *__restrict__ bug, const double *__restrict__ lbg,
    const double *__restrict__ ubg, double *__restrict__ xg, double *__restrict__ lamg, uint32_t *__restrict__ actg,
    uint32_t *__restrict__ lowg, int32_t *__restrict__ statg, int32_t *__restrict__ itg, int n, int m, int mg, int meq,
    long long batch, int max_iter, double feas_tol, long long strideH, long long strideA) {
  __shared__ double lds[QPB * SLOT];
  gi_group<MR, N16, FULL, false, true, true, true, 0, true>(lds, Hg, fg, Gg, bug, xg, lamg, actg, statg, itg, n, m,
                                                            batch, max_iter, feas_tol, 0, nullptr, blockIdx.x, meq,
                                                            strideH, strideA, blg, lowg, mg, ubg, lbg);
}

// qpb_factor_shared's kernel: one workgroup, whose first row factors the one
// problem with this form's own load and sweep (gi_group with FM = 1)
template <int MR, bool N16, bool FULL>
__global__ __launch_bounds__(64) void gi_dense_factor_kernel(const double *__restrict__ Hg,
                                                             const double *__restrict__ Ag, double *__restrict__ fac,
                                                             int32_t *__restrict__ fstatus, int n, int m) {
  __shared__ double lds[QPB * SLOT];
  gi_group<MR, N16, FULL, false, false, false, false, 1>(lds, Hg, nullptr, Ag, nullptr, fac, nullptr, nullptr, fstatus,
                                                         nullptr, n, m, 1, 0, 0.0, 0, nullptr, 0);
}

// qpb_solve_factored's form: gi_group with FM = 2, with or without equality rows
template <int MR, bool N16, bool FULL, bool EQ, int OCC>
__global__ __launch_bounds__(64, OCC) void gi_dense_factored_kernel(
    const double *__restrict__ facg, const double *__restrict__ fg, const double *__restrict__ bg,
    double *__restrict__ xg, double *__restrict__ lamg, uint32_t *__restrict__ actg, int32_t *__restrict__ statg,
    int32_t *__restrict__ itg, int n, int m, int meq, long long batch, int max_iter, double feas_tol) {
  __shared__ double lds[QPB * SLOT];
  static_assert(fct::layout(16, 16 * MR).mr == MR);
  gi_group<MR, N16, FULL, false, EQ, true, false, 2>(lds, facg, fg, facg + fct::layout(n, m).A, bg, xg, lamg, actg,
                                                     statg, itg, n, m, batch, max_iter, feas_tol, 0, nullptr,
                                                     blockIdx.x, meq, 0, 0);
}

// qpb_solve_range_factored's form: gi_group with RG and FM = 2 (meq an argument)
template <int MR, bool N16, bool FULL, int OCC>
__global__ __launch_bounds__(64, OCC) void gi_dense_range_factored_kernel(
    const double *__restrict__ facg, const double *__restrict__ fg, const double *__restrict__ blg,
    const double *__restrict__ bug, double *__restrict__ xg, double *__restrict__ lamg, uint32_t *__restrict__ actg,
    uint32_t *__restrict__ lowg, int32_t *__restrict__ statg, int32_t *__restrict__ itg, int n, int m, int meq,
    long long batch, int max_iter, double feas_tol) {
  __shared__ double lds[QPB * SLOT];
  static_assert(fct::layout(16, 16 * MR).mr == MR);
  gi_group<MR, N16, FULL, false, true, true, true, 2>(lds, facg, fg, facg + fct::layout(n, m).A, bug, xg, lamg, actg,
                                                      statg, itg, n, m, batch, max_iter, feas_tol, 0, nullptr,
                                                      blockIdx.x, meq, 0, 0, blg, lowg);
}

}  // namespace qpb

// launcher used by qpb_api.hip
extern "C" hipError_t qpb_launch_gi(const qpb_desc *d, const double *H, const double *f, const double *A,
                                    const double *b, double *x, double *lam, uint32_t *active,
                                    int32_t *status, int32_t *iters, hipStream_t stream) {
  const long long blocks = (d->batch + qpb::QPB - 1) / qpb::QPB;
  const auto [max_iter, tol] = qpb_resolve_limits(d);
  // every form at 3 waves per SIMD (VGPRs and LDS)
  qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto FULL) {
    hipLaunchKernelGGL((qpb::gi_dense_kernel<MR(), N16(), FULL(), false, 3>), dim3((unsigned)blocks), dim3(64), 0,
                       stream, H, f, A, b, x, lam, active, status, iters, d->n, d->m, (long long)d->batch, max_iter,
                       tol, d->flags);
  });
  return hipGetLastError();
}

// qpb_solve_eq, n <= 16 and m <= 32: the same six forms with equality rows
extern "C" hipError_t qpb_launch_gi_eq(const qpb_desc *d, int meq, const double *H, const double *f, const double *A,
                                       const double *b, double *x, double *lam, uint32_t *active, int32_t *status,
                                       int32_t *iters, hipStream_t stream) {
  const long long blocks = (d->batch + qpb::QPB - 1) / qpb::QPB;
  const auto [max_iter, tol] = qpb_resolve_limits(d);
  qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto FULL) {
    hipLaunchKernelGGL((qpb::gi_dense_eq_kernel<MR(), N16(), FULL(), qpb::kEqOcc>), dim3((unsigned)blocks), dim3(64),
                       0, stream, H, f, A, b, x, lam, active, status, iters, d->n, d->m, meq, (long long)d->batch,
                       max_iter, tol);
  });
  return hipGetLastError();
}

// diagnostic: per-section wave ticks of the n=16, 16<m<=32 kernel (sections[256][20])
extern "C" hipError_t qpb_launch_gi_sections(const qpb_desc *d, const double *H, const double *f, const double *A,
                                             const double *b, double *x, double *lam, uint32_t *active,
                                             int32_t *status, int32_t *iters, unsigned long long *sections,
                                             hipStream_t stream) {
  const long long blocks = (d->batch + qpb::QPB - 1) / qpb::QPB;
  const auto [max_iter, tol] = qpb_resolve_limits(d);
  if (d->n != 16 || d->m <= 16) return hipErrorInvalidValue;
#ifdef QPB_WAVE_TRACE
  // the diagnostic build launches the shipped kernel and writes 8 words per
  // wave: the caller's buffer holds 8 * ceil(batch / 4) (tools/wave_timeline.py)
  if (d->m == 32) {
    hipLaunchKernelGGL((qpb::gi_dense_kernel<2, true, true, false, 3>), dim3((unsigned)blocks), dim3(64), 0, stream,
                       H, f, A, b, x, lam, active, status, iters, d->n, d->m, (long long)d->batch, max_iter, tol,
                       d->flags, sections);
    return hipGetLastError();
  }
#endif
  hipLaunchKernelGGL((qpb::gi_dense_kernel<2, true, false, true>), dim3((unsigned)blocks), dim3(64), 0, stream, H, f,
                     A, b, x, lam, active, status, iters, d->n, d->m, (long long)d->batch, max_iter, tol, d->flags,
                     sections);
  return hipGetLastError();
}

// qpb_solve_shared, n <= 16 and m <= 32: the six forms with run-time QP strides
// of H and A (0: one copy for the batch), plain (meq == 0) and EQ
extern "C" hipError_t qpb_launch_gi_shared(const qpb_desc *d, int meq, long long strideH, long long strideA,
                                           const double *H, const double *f, const double *A, const double *b,
                                           double *x, double *lam, uint32_t *active, int32_t *status, int32_t *iters,
                                           hipStream_t stream) {
  const long long blocks = (d->batch + qpb::QPB - 1) / qpb::QPB;
  const auto [max_iter, tol] = qpb_resolve_limits(d);
  qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto FULL) {
    if (meq > 0)
      hipLaunchKernelGGL((qpb::gi_dense_shared_kernel<MR(), N16(), FULL(), true, qpb::kEqOcc>),
                         dim3((unsigned)blocks), dim3(64), 0, stream, H, f, A, b, x, lam, active, status, iters, d->n,
                         d->m, meq, (long long)d->batch, max_iter, tol, strideH, strideA);
    else
      hipLaunchKernelGGL((qpb::gi_dense_shared_kernel<MR(), N16(), FULL(), false, 3>), dim3((unsigned)blocks),
                         dim3(64), 0, stream, H, f, A, b, x, lam, active, status, iters, d->n, d->m, 0,
                         (long long)d->batch, max_iter, tol, strideH, strideA);
  });
  return hipGetLastError();
}

// qpb_solve_range, n <= 16 and 1 <= m <= 32: the six forms with two-sided rows,
// equality rows 0 .. meq-1 and run-time QP strides of H and A
extern "C" hipError_t qpb_launch_gi_range(const qpb_desc *d, int meq, long long strideH, long long strideA,
                                          const double *H, const double *f, const double *A, const double *bl,
                                          const double *bu, double *x, double *lam, uint32_t *active,
                                          uint32_t *lower, int32_t *status, int32_t *iters, hipStream_t stream) {
  const long long blocks = (d->batch + qpb::QPB - 1) / qpb::QPB;
  const auto [max_iter, tol] = qpb_resolve_limits(d);
  qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto FULL) {
    hipLaunchKernelGGL((qpb::gi_dense_range_kernel<MR(), N16(), FULL(), qpb::kEqOcc>), dim3((unsigned)blocks),
                       dim3(64), 0, stream, H, f, A, bl, bu, x, lam, active, lower, status, iters, d->n, d->m, meq,
                       (long long)d->batch, max_iter, tol, strideH, strideA);
  });
  return hipGetLastError();
}

// qpb_solve_range_box, n <= 16 and d->m = mg + n <= 32: the six forms by all the
// rows, the last n of them the variables' bounds (mg >= 0; G unread at mg == 0)
extern "C" hipError_t qpb_launch_gi_range_box(const qpb_desc *d, int mg, int meq, long long strideH, long long strideA,
                                              const double *H, const double *f, const double *G, const double *bl,
                                              const double *bu, const double *lb, const double *ub, double *x,
                                              double *lam, uint32_t *active, uint32_t *lower, int32_t *status,
                                              int32_t *iters, hipStream_t stream) {
  const long long blocks = (d->batch + qpb::QPB - 1) / qpb::QPB;
  const auto [max_iter, tol] = qpb_resolve_limits(d);
  qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto FULL) {
    hipLaunchKernelGGL((qpb::gi_dense_range_box_kernel<MR(), N16(), FULL(), qpb::kEqOcc>), dim3((unsigned)blocks),
                       dim3(64), 0, stream, H, f, G, bl, bu, lb, ub, x, lam, active, lower, status, iters, d->n, d->m,
                       mg, meq, (long long)d->batch, max_iter, tol, strideH, strideA);
  });
  return hipGetLastError();
}

// qpb_factor_shared, n <= 16 and m <= 32: one launch of one workgroup
extern "C" hipError_t qpb_launch_gi_factor(int n, int m, const double *H, const double *A, double *fac,
                                           int32_t *fstatus, hipStream_t stream) {
  qpb::row16::dispatch_form(n, m, [&](auto MR, auto N16, auto FULL) {
    hipLaunchKernelGGL((qpb::gi_dense_factor_kernel<MR(), N16(), FULL()>), dim3(1), dim3(64), 0, stream, H, A, fac,
                       fstatus, n, m);
  });
  return hipGetLastError();
}

// qpb_solve_factored, n <= 16 and m <= 32: the six forms on a factor buffer,
// plain (meq == 0) and EQ
extern "C" hipError_t qpb_launch_gi_factored(const qpb_desc *d, int meq, const double *fac, const double *f,
                                             const double *b, double *x, double *lam, uint32_t *active,
                                             int32_t *status, int32_t *iters, hipStream_t stream) {
  const long long blocks = (d->batch + qpb::QPB - 1) / qpb::QPB;
  const auto [max_iter, tol] = qpb_resolve_limits(d);
  qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto FULL) {
    if (meq > 0)
      hipLaunchKernelGGL((qpb::gi_dense_factored_kernel<MR(), N16(), FULL(), true, qpb::kEqOcc>),
                         dim3((unsigned)blocks), dim3(64), 0, stream, fac, f, b, x, lam, active, status, iters, d->n,
                         d->m, meq, (long long)d->batch, max_iter, tol);
    else
      hipLaunchKernelGGL((qpb::gi_dense_factored_kernel<MR(), N16(), FULL(), false, 3>), dim3((unsigned)blocks),
                         dim3(64), 0, stream, fac, f, b, x, lam, active, status, iters, d->n, d->m, 0,
                         (long long)d->batch, max_iter, tol);
  });
  return hipGetLastError();
}

// qpb_solve_range_factored, n <= 16 and 1 <= m <= 32: the six forms with
// two-sided rows and equality rows 0 .. meq-1 on a factor buffer
extern "C" hipError_t qpb_launch_gi_range_factored(const qpb_desc *d, int meq, const double *fac, const double *f,
                                                   const double *bl, const double *bu, double *x, double *lam,
                                                   uint32_t *active, uint32_t *lower, int32_t *status, int32_t *iters,
                                                   hipStream_t stream) {
  const long long blocks = (d->batch + qpb::QPB - 1) / qpb::QPB;
  const auto [max_iter, tol] = qpb_resolve_limits(d);
  qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto FULL) {
    hipLaunchKernelGGL((qpb::gi_dense_range_factored_kernel<MR(), N16(), FULL(), qpb::kEqOcc>),
                       dim3((unsigned)blocks), dim3(64), 0, stream, fac, f, bl, bu, x, lam, active, lower, status,
                       iters, d->n, d->m, meq, (long long)d->batch, max_iter, tol);
  });
  return hipGetLastError();
}
