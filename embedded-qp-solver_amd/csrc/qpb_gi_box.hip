// qpb_gi_box.hip -- batched box-constrained QP kernel for gfx950 (n <= 16).
//
//   min 1/2 x^T H x + f^T x   s.t.   lb <= x <= ub        (fp64, one QP per 16 lanes)
//
// The constraint class of the reference's only constrained solver, admm()
// (qp_solvers/qp_solvers.c:146-319, box bounds config.h:29-30), solved exactly:
// the dual active-set method of qpb_gi.hip (Goldfarb & Idnani) on the implicit
// A = [I; -I], b = [ub; -lb] -- SURVEY.md §8b's BOX constraint kind and §8d's
// box fast path (2,824 algorithmic bytes per QP at n = 16 instead of 6,920).
// With A implicit the kernel is qpb_gi.hip with three simplifications:
//   D = A L^{-T} = [L^{-T}; -L^{-T}]: lane l keeps ONE row, row l of L^{-T}
//     (the setup sweep starts it from e_l); the lower bound's row is its
//     negative, so the slack step's product and the Householder reflection
//     touch 16 values per lane instead of 32, and every row has norm 1.
//   the exchange row: the owner lane writes its only row (no row select);
//     readers fold in the sign of the selected bound (the reflection is
//     sign-free: v v^T with v = sgn v').
//   x = -H^{-1} (f + lambda_u - lambda_l): no rows of A to read back.
// Constraint numbering inside the kernel: row l (upper bound of x_l) and row
// 16 + l (lower bound); outputs use qpb_solve's m = 2n numbering (upper bounds
// 0..n-1, lower bounds n..2n-1), i.e. A = [I; -I] row order.  Infinite bounds
// (or a NULL lb / ub) are absent constraints: their slack is +inf.
// The QP's LDS slot (L | R, its column 0 the exchange row | s_p) and the steps
// the kernel has in common with gi_dense are qpb_row16.h's.
#include <type_traits>

#include "qpb_factor.h"  // the box factor buffer of qpb_factor_box / qpb_solve_box_factored
#include "qpb_launch.h"  // with qpb.h
#include "qpb_row16.h"

namespace qpb {
namespace box {
using namespace row16;

// N16: n == 16 (coalesced H loads through an LDS transpose); otherwise the
// rows are padded with the identity and the padded variables get no bounds
// SH (qpb_solve_box_shared): the QP stride of H, in doubles, is the one
// trailing argument that only this form has, the run-time strideH -- 0 for one
// H that the whole batch shares, or n n.  H is read through the QP's base
// pointer alone (the N16 form's coalesced 16-byte loads and LDS transpose are
// the same code on the one matrix: every QP of the wave then reads the same two
// rows per instruction), so the outputs are the other form's bit for bit.
// Without SH the pack is empty, and the signature and the code object stay as
// they were.
// The factor forms (qpb_factor.h, bxfct, has the buffer) ride in the same pack:
// BoxFactorOut (qpb_factor_box): ONE problem (batch 1, no f and no bounds), the
// kernel's own load and sweep, then L, the lane's row of L^-T, its squared norm
// and what the sweep found go to the buffer, and nothing else runs.
// BoxFactorIn (qpb_solve_box_factored): no H is loaded and nothing is swept --
// the lane's rows of L and of L^-T come from the buffer with 16-byte loads at
// consecutive addresses, fn2 from the stored squared norm; y = L^-1 f is a
// lane-parallel forward substitution whose steps also accumulate e = (L^-T y)_l
// (both by DPP-fused FMAs that read y_k from lane k), and the slacks are
// ub + e and -lb - e.  From the active-set loop on the code is the other forms'.
struct BoxFactorOut {
  double *fac;
  int32_t *fstatus;  // may be NULL
};
struct BoxFactorIn {
  const double *fac;
};
template <bool N16, bool SH = false, class... STR>
__global__ __launch_bounds__(64, 3) void gi_box_kernel(const double *__restrict__ Hg, const double *__restrict__ fg,
                                                       const double *__restrict__ lbg, const double *__restrict__ ubg,
                                                       double *__restrict__ xg, double *__restrict__ lamg,
                                                       uint32_t *__restrict__ actg, int32_t *__restrict__ statg,
                                                       int32_t *__restrict__ itg, int n, long long batch,
                                                       int max_iter, double feas_tol, STR... strideH) {
  constexpr bool FO = (std::is_same_v<STR, BoxFactorOut> || ...), FI = (std::is_same_v<STR, BoxFactorIn> || ...);
  static_assert(sizeof...(STR) == ((SH || FO || FI) ? 1 : 0) && (FO || FI || (std::is_same_v<STR, long long> && ...)) &&
                    !(SH && (FO || FI)),
                "the shared form alone takes the stride, a factor form its buffer");
  __shared__ double lds[QPB * SLOT];
  const int l = threadIdx.x & (NL - 1);
  const int slot = threadIdx.x >> 4;
  const auto [live, g] = ragged_qp(blockIdx.x, slot, batch);
  if constexpr (N16) n = NL;
  double *base = slot_base(lds, slot);
  double *Lp = base + OFF_L;
  double *R = base + OFF_R;
  double *xch = R;  // the exchange row in R's column 0 (never read by the back substitution)
  double *xsp = base + OFF_XCH;

  // ------------------------------------------------------------------ load
  const bool var = N16 || l < n;  // lane l carries variable l
  const int lc = var ? l : n - 1;
  [[maybe_unused]] const double *Hq;
  if constexpr (SH)
    Hq = Hg + g * (strideH + ...);
  else
    Hq = Hg + g * (long long)n * n;
  double fv0 = 0.0;
  if constexpr (!FO) fv0 = fg[g * n + lc];  // the factor kernel has no f
  const double fv = fv0;
  const double ubv = ubg ? ubg[g * n + lc] : kInf;
  const double lbv = lbg ? lbg[g * n + lc] : -kInf;
  double Lr[NL];  // row l of H, becomes row l of L
  double E[NL];   // row l of D = L^{-T}, from e_l
  [[maybe_unused]] double fdn = 0.0;  // FI: |row l of L^-T|^2 from the buffer
  [[maybe_unused]] bool fspd = true;  // FI: the buffer's H was positive definite
  constexpr int oFL = bxfct::kHdr, oFD = oFL + NL * NL, oFN = oFD + NL * NL;
  static_assert(bxfct::layout(NL).L == oFL && bxfct::layout(1).D == oFD && bxfct::layout(NL).dn2 == oFN &&
                bxfct::layout(1).size == oFN + NL && bxfct::layout(NL).np == NL);
  if constexpr (FI) {
    // the buffer in place of H: 16 bytes per lane at consecutive addresses,
    // the same for the wave's four QPs and every other wave
    const double *facg = [](BoxFactorIn a) { return a; }(strideH...).fac;
    fspd = facg[0] != (double)QPB_NOT_SPD;
#pragma unroll
    for (int t = 0; t < NL / 2; ++t) {
      const double2 v = *reinterpret_cast<const double2 *>(&facg[oFL + (t * NL + l) * 2]);
      Lr[2 * t] = v.x;
      Lr[2 * t + 1] = v.y;
    }
#pragma unroll
    for (int t = 0; t < NL / 2; ++t) {
      const double2 v = *reinterpret_cast<const double2 *>(&facg[oFD + (t * NL + l) * 2]);
      E[2 * t] = v.x;
      E[2 * t + 1] = v.y;
    }
    fdn = facg[oFN + l];
  } else if constexpr (N16) {
    // one instruction reads two whole rows of each of the wave's 4 QPs; the
    // rows reach their owner lanes through a transpose in this QP's LDS slot
    // (L and R are written after the factorisation)
    const int hr = l >> 3, hc = 2 * (l & 7);
    double2 hv[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) hv[t] = *reinterpret_cast<const double2 *>(&Hq[(2 * t + hr) * NL + hc]);
    asm volatile("" ::"v"(fv), "v"(ubv), "v"(lbv));
#pragma unroll
    for (int t = 0; t < 8; ++t) asm volatile("" ::"v"(hv[t].x), "v"(hv[t].y));
    wave_lds_sync();
#pragma unroll
    for (int t = 0; t < 8; ++t) *reinterpret_cast<double2 *>(&base[(2 * t + hr) * RS + hc]) = hv[t];
    wave_lds_sync();
    lds_row16(&base[l * RS], Lr);
    wave_lds_sync();
  } else {
#pragma unroll
    for (int j = 0; j < NL; ++j) Lr[j] = h_padded(Hq, l, lc, n, j);
  }
  if constexpr (!FI) {
#pragma unroll
    for (int j = 0; j < NL; ++j) E[j] = l == j ? 1.0 : 0.0;
  }
  // b of the two rows: ub (x_l <= ub_l) and -lb (-x_l <= -lb_l)
  const double bu = var ? ubv : kInf, bl = var ? -lbv : kInf;
  // violation thresholds of the (unit-norm) rows; -inf for an absent bound
  const double thu = -feas_tol * (1.0 + __builtin_fabs(bu)), thl = -feas_tol * (1.0 + __builtin_fabs(bl));
  const double fl = var ? fv : 0.0;

  // ---- H = L L^T, D = L^{-T} (row l from e_l), y = L^{-1} f in one
  // right-looking sweep (qpb_gi.hip, one D row per lane); e = D y accumulates
  // alongside (y_k is final at step k)
  bool spd = true;
  double ya = fl, ey = 0.0;
  if constexpr (FI) {
    // ---- y = L^{-1} f and e = (L^{-T} y)_l from the stored L and L^{-T}, on the
    // negated accumulator na = -(f - sum L y): step k forms t = na ninv, which is
    // y_k on lane k (ninv = -1 / L[l][l]), and both FMAs of the step read it from
    // lane k by their own DPP broadcast.  t is a VALU result read through DPP:
    // dpp_ready issues the wait states.  Lane k's own na becomes 0 at step k and
    // is dead from there on, like the entries of its row of L right of the
    // diagonal (zero in the buffer).
    spd = fspd;
    store_l(Lp, l, Lr);  // for the final solves
    const double ninv = -rcp1(Lp[lrow(l) + l]);
    wave_lds_sync();
    double na = -ya;
    unroll<NL>([&](auto K) {
      constexpr int k = K;
      const double t = na * ninv;
      dpp_ready(t);
      fmac_bc<k>(ey, t, E[k]);
      fmac_bc<k>(na, t, Lr[k]);
    });
  }
  if constexpr (!FI) unroll<NL>([&](auto K) {
    constexpr int k = K;
    __builtin_amdgcn_sched_barrier(0);
    const double akk = bc<k>(Lr[k]);
    spd = spd && (akk > 0.0);
    const double ik = rsq1(akk);
    const double ik2 = ik * ik;
    const double nc = -(Lr[k] * ik2);
    const double e = E[k];
    const double ne2 = -(e * ik2);
    E[k] = e * ik;
    unroll<NL - 1 - k>([&](auto J) {
      constexpr int j = k + 1 + J;
      fmac_bc<k>(E[j], Lr[j], ne2);
      fmac_bc<k>(Lr[j], Lr[j], nc);
    });
    Lr[k] *= ik;
    const double c = -nc;
    const double fk = bc<k>(ya);
    ya = __builtin_fma(-c, fk, ya);
    ey = __builtin_fma(E[k], fk * ik, ey);
  });
  if constexpr (!FI) {
    __builtin_amdgcn_sched_barrier(0);
    store_l(Lp, l, Lr);  // for the final solves
  }
  // slacks of the unconstrained minimiser x0 = -L^{-T} y: b + D y per row
  double su = bu + ey, sl = bl - ey;
  // |D[l, q:]|^2, the free part of both of the lane's rows (scale of the
  // selection key, as qpb_gi.hip)
  double dn2;
  if constexpr (FI) dn2 = fdn;
  else dn2 = dot2<NL>([&](int j) { return E[j]; }, [&](int j) { return E[j]; });
  if constexpr (FO) {
    // ---- the factor kernel ends here: the live row (QP 0) writes the buffer
    const BoxFactorOut fo = [](BoxFactorOut a) { return a; }(strideH...);
    const int found = spd ? QPB_OK : QPB_NOT_SPD;
    if (live) {
      double *fac = fo.fac;
      if (l < bxfct::kHdr) fac[l] = l == 0 ? (double)found : l == 1 ? (double)n : l == 2 ? (double)NL : 0.0;
      if (l == 0 && fo.fstatus) fo.fstatus[0] = found;
#pragma unroll
      for (int t = 0; t < NL / 2; ++t) {  // zero right of the diagonal (the sweep leaves dead values there)
        *reinterpret_cast<double2 *>(&fac[oFL + (t * NL + l) * 2]) =
            make_double2(2 * t <= l ? Lr[2 * t] : 0.0, 2 * t + 1 <= l ? Lr[2 * t + 1] : 0.0);
        *reinterpret_cast<double2 *>(&fac[oFD + (t * NL + l) * 2]) = make_double2(E[2 * t], E[2 * t + 1]);
      }
      fac[oFN + l] = dn2;
    }
    return;
  }
  float fn2 = (float)dn2;

  // ------------------------------------------------------ active-set loop
  // zeroed in pairs at lane-rotated positions (the same position in every
  // lane's column would be an 8-way bank conflict per store)
#pragma unroll
  for (int j = 0; j < NL; j += 2)
    *reinterpret_cast<double2 *>(&R[l * NL + ((j + 2 * l) & (NL - 1))]) = make_double2(0.0, 0.0);
  int q = 0;
  double um = 0.0;  // multiplier of active position l
  int iam = -1;     // constraint (0..15 upper, 16..31 lower) at active position l
  double rdg = 0.0, invRd = 0.0;
  bool actu = false, actl = false;
  int status = spd ? QPB_MAX_ITER : QPB_NOT_SPD;
  bool done = !spd;
  bool selecting = true;
  int p = 0;
  double up = 0.0;
  int it = 0;
  wave_lds_sync();
  while (!done && it < max_iter) {
    ++it;
    if (selecting) {
      // violated bounds (rows of unit norm) ranked by dual steepest edge,
      // -s / |D[l, q:]| as in qpb_gi.hip (the same choices as the dense path
      // on A = [I; -I]): fp32 keys with the row in the low 5 bits, DPP-fused max
      // (fn2 >= 0, clamped where it shrinks; the 2^-100 floor keeps a violated
      // bound's key nonzero -- 0 is "none violated" -- when the ratio underflows)
      const float rf = __builtin_amdgcn_rsqf(fn2);
      const uint32_t ku = (__float_as_uint(__builtin_fmaf((float)(-su), rf, 0x1p-100f)) & ~31u) | (uint32_t)l;
      const uint32_t kl = (__float_as_uint(__builtin_fmaf((float)(-sl), rf, 0x1p-100f)) & ~31u) | (uint32_t)(l + NL);
      uint32_t key = (!actu && su < thu) ? ku : 0u;
      key = (!actl && sl < thl && kl > key) ? kl : key;
      key = row_max_u32(key);
      if (key == 0u) {
        status = QPB_OK;
        done = true;
        break;
      }
      p = (int)(key & 31u);
      up = 0.0;
      selecting = false;
    }
    const int qmax = __builtin_elementwise_min(wave_max4(q), NL);
    const int owner = p & (NL - 1);
    const double sgn = p < NL ? 1.0 : -1.0;  // D[p,:] = sgn * (row `owner` of L^{-T})
    if (l == owner) {
#pragma unroll
      for (int j = 0; j < NL; j += 2) *reinterpret_cast<double2 *>(&xch[j]) = make_double2(E[j], E[j + 1]);
      *xsp = p < NL ? su : sl;
    }
    wave_lds_sync();
    const double wl = xch[l];
    const double wq = xch[q & (NL - 1)];  // q == 16: only used by an ADD, impossible then
    const double sp = *xsp;
    // the selected row with its active columns zeroed, entry j at lane j
    // (d2 = sgn * w2): the products below take it by DPP broadcast
    const double w2 = l >= q ? wl : 0.0;
    dpp_ready(w2);
    const double Dpl = sgn * wl, Dpq = sgn * wq;
    const double dl = -Dpl;
    const double nd2 = row_sum(l >= q ? wl * wl : 0.0);  // |d2|^2
    const double dd = row_sum(wl * wl);                  // |D[p,:]|^2

    // ---- r = R^{-1} d1 (lane-parallel back substitution, DPP-fused FMAs)
    double rm = 0.0;
    if (qmax > 0) {
      const double ninv = -invRd;
      double nacc = (l < q) ? Dpl : 0.0;
      unroll<NL>([&](auto JJ) { back_subst_step<NL - 1 - JJ>(R, l, qmax, nacc, ninv); });
      rm = nacc * ninv;
    }
    // ---- step lengths: exact ratio minimum, then the lowest position reaching it
    double t1 = kBig;
    int k = 0;
    if (qmax > 0) {
      const double ratio = um * rcp1(rm);
      const bool cand = l < q && rm > 0.0;
      t1 = row_min(cand ? ratio : kBig);
      k = (int)row_min_u32(cand && ratio == t1 ? (uint32_t)l : 31u) & (NL - 1);
    }
    const double ir = rsq1(nd2);
    const double t2 = (nd2 > kDepTol * dd) ? -sp * (ir * ir) : kBig;
    const double t = t1 < t2 ? t1 : t2;
    if (!(t < kBig)) {
      status = QPB_INFEASIBLE;
      done = true;
      break;
    }
    double u = 0.0;  // D[l,:] . d2
    if (t2 < kBig) {  // slacks s -= t D[:, q:] d2: the upper row's product, negated for the lower
      double a0 = 0.0, a1 = 0.0;
      unroll<NL>([&](auto J) {
        constexpr int j = J;
        fmac_bc<j>(j % 2 ? a1 : a0, w2, E[j]);
      });
      u = sgn * (a0 + a1);
      su = __builtin_fma(t, u, su);
      sl = __builtin_fma(-t, u, sl);
    }
    pin(su);
    pin(sl);
    um = __builtin_fma(-t, rm, um);
    up += t;

    if (t2 <= t1) {
      // ---------------- ADD p: Householder on columns q.. of D.  v = d2 +
      // alpha e_q = sgn (w2 + sgn alpha e_q), and the reflection I - beta v v^T
      // only sees v v^T, so the unsigned v' = w2 + sgn alpha e_q is formed in LDS
      const double nrm = nd2 * ir;
      const double alpha = Dpq <= 0.0 ? -nrm : nrm;
      const double beta = ir * rcp1(nrm + __builtin_fabs(Dpq));
      const double ia = Dpq <= 0.0 ? -ir : ir;  // 1 / alpha
      // the reflection maps e_q to -d2 / alpha: column q of the new D is
      // -u / alpha, and it leaves the free part of the row
      const float cq = (float)(u * ia);
      fn2 = __builtin_fmaxf(__builtin_fmaf(-cq, cq, fn2), 0.0f);
      const double v = w2 + (l == q ? sgn * alpha : 0.0);
      dpp_ready(v);
      double a0 = 0.0, a1 = 0.0;
      unroll<NL>([&](auto J) {
        constexpr int j = J;
        fmac_bc<j>(j % 2 ? a1 : a0, v, E[j]);
      });
      const double nw = -beta * (a0 + a1);
      unroll<NL>([&](auto J) {
        constexpr int j = J;
        fmac_bc<j>(E[j], v, nw);
      });
      R[q * NL + l] = (l < q) ? dl : 0.0;
      if (l == q) {
        rdg = alpha;
        invRd = ia;
        iam = p;
        um = up;
      }
      if (l == owner) {
        actu = actu || p < NL;
        actl = actl || p >= NL;
      }
      ++q;
      selecting = true;
    } else {
      // ---------------- DROP active position k (as qpb_gi.hip)
      const int c = __shfl(iam, k, NL);
      if (l == (c & (NL - 1))) {
        actu = actu && c >= NL;
        actl = actl && c < NL;
      }
      const double un = __shfl(um, (l + 1) & (NL - 1), NL);
      const int in = __shfl(iam, (l + 1) & (NL - 1), NL);
      if (l >= k && l < q - 1) {
        um = un;
        iam = in;
      } else if (l == q - 1) {
        um = 0.0;
        iam = -1;
      }
      // full R (diagonal put back), delete column k (lane l owns column l)
      wave_lds_sync();
      if (l < q) R[l * NL + l] = rdg;
      // lane l copies column l+1 whole (one pass: in-order DS, every read
      // precedes every write), pairs at lane-rotated positions (conflict-free)
      {
        double2 col[NL / 2];
#pragma unroll
        for (int t = 0; t < NL / 2; ++t)
          col[t] = *reinterpret_cast<const double2 *>(&R[((l + 1) & (NL - 1)) * NL + ((2 * t + 2 * l) & (NL - 1))]);
        wave_lds_sync();
        if (l >= k && l < q - 1) {
#pragma unroll
          for (int t = 0; t < NL / 2; ++t) *reinterpret_cast<double2 *>(&R[l * NL + ((2 * t + 2 * l) & (NL - 1))]) = col[t];
        } else if (l == q - 1) {
#pragma unroll
          for (int t = 0; t < NL / 2; ++t)
            *reinterpret_cast<double2 *>(&R[l * NL + ((2 * t + 2 * l) & (NL - 1))]) = make_double2(0.0, 0.0);
        }
      }
      // Givens rotations restore the upper-triangular R (lane j keeps rotation
      // j's parameters for the D update, which reads them by DPP) ...
      double gc = 0.0, gs = 0.0;
      for (int j = k; j < q - 1; ++j) {
        wave_lds_sync();
        const double a = R[j * NL + j], bb = R[j * NL + j + 1];
        const double irr = rsq1(__builtin_fma(a, a, bb * bb));
        const double cj = a * irr, sj = bb * irr;
        const double rj = R[l * NL + j], rj1 = R[l * NL + j + 1];
        wave_lds_sync();
        if (l >= j && l < q - 1) {
          R[l * NL + j] = __builtin_fma(cj, rj, sj * rj1);
          R[l * NL + j + 1] = (l == j) ? 0.0 : __builtin_fma(-sj, rj, cj * rj1);
        }
        if (l == j) {
          gc = cj;
          gs = sj;
        }
      }
      wave_lds_sync();
      R[l * NL + q - 1] = 0.0;
      // ... and the same rotations on D's columns
      unroll<NL - 1>([&](auto JJ) {
        constexpr int j = JJ;
        if (j + 1 < qmax && j >= k && j < q - 1) {
          const double cj = bc<j>(gc), sj = bc<j>(gs);
          rotate_pair<j>(E, cj, sj);
        }
      });
      --q;
      // column q (after the rotations) joins the free part: recompute
      {
        float a0 = 0.0f, a1 = 0.0f;
        unroll<NL>([&](auto J) {
          constexpr int j = J;
          const float e = (float)E[j];
          if constexpr (j % 2 == 0) a0 = __builtin_fmaf(e, j >= q ? e : 0.0f, a0);
          if constexpr (j % 2 == 1) a1 = __builtin_fmaf(e, j >= q ? e : 0.0f, a1);
        });
        fn2 = a0 + a1;
      }
      const double dg = take_diagonal(R, l, q);
      rdg = dg;
      invRd = (l < q) ? rcp1(dg) : 0.0;
    }
    wave_lds_sync();
  }

  // ------------------------------------------------------------- outputs
  // multipliers by constraint (row l: upper bound of x_l, row 16 + l: lower)
  double *lamb = R;  // 32 over the dead R; the solves capture in R[32:48]
  double *xcap = R + 2 * NL;
  wave_lds_sync();
  lamb[l] = 0.0;
  lamb[l + NL] = 0.0;
  wave_lds_sync();
  if (l < q && iam >= 0) lamb[iam] = dual_out(um);  // lam >= 0: a tie's -eps written as 0
  wave_lds_sync();
  const double lu = lamb[l], ll = lamb[l + NL];
  wave_lds_sync();
  // x = -H^{-1} (f + A^T lam), A^T lam = lam_u - lam_l
  const double invd = rcp1(Lp[lrow(l) + l]);
  double Lrow[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) Lrow[j] = Lp[lrow(l) + j];
  wave_lds_sync();
  const double xl = solve_x(fl + lu - ll, invd, Lrow, Lp, l, xcap);
  status = x_status(status, xl);
  if (live && var) {
    xg[g * n + l] = xl;
    lamg[g * 2 * n + l] = lu;
    lamg[g * 2 * n + n + l] = ll;
  }
  const int sh = (threadIdx.x & 63) & ~(NL - 1);
  const uint32_t wu = (uint32_t)((__ballot(actu) >> sh) & 0xFFFFull);
  const uint32_t wlo = (uint32_t)((__ballot(actl) >> sh) & 0xFFFFull);
  if (live && l == 0) {
    actg[g] = wu | (wlo << n);  // m = 2n <= 32: one word, A = [I; -I] row order
    statg[g] = status;
    if (itg) itg[g] = it;
  }
}

}  // namespace box
}  // namespace qpb

extern "C" hipError_t qpb_launch_gi_box(const qpb_desc *d, const double *H, const double *f, const double *lb,
                                        const double *ub, double *x, double *lam, uint32_t *active, int32_t *status,
                                        int32_t *iters, hipStream_t stream) {
  const long long blocks = (d->batch + qpb::box::QPB - 1) / qpb::box::QPB;
  const auto [max_iter, tol] = qpb_resolve_limits(d);
  const auto kernel = d->n == 16 ? qpb::box::gi_box_kernel<true> : qpb::box::gi_box_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64), 0, stream, H, f, lb, ub, x, lam, active, status,
                     iters, d->n, (long long)d->batch, max_iter, tol);
  return hipGetLastError();
}

// qpb_solve_box_shared for n <= 16: the SH forms, H's QP stride at run time (0:
// one copy for the batch, or n n)
extern "C" hipError_t qpb_launch_gi_box_shared(const qpb_desc *d, const double *H, const double *f, const double *lb,
                                               const double *ub, double *x, double *lam, uint32_t *active,
                                               int32_t *status, int32_t *iters, long long strideH,
                                               hipStream_t stream) {
  const long long blocks = (d->batch + qpb::box::QPB - 1) / qpb::box::QPB;
  const auto [max_iter, tol] = qpb_resolve_limits(d);
  const auto kernel = d->n == 16 ? qpb::box::gi_box_kernel<true, true, long long>
                                 : qpb::box::gi_box_kernel<false, true, long long>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64), 0, stream, H, f, lb, ub, x, lam, active, status,
                     iters, d->n, (long long)d->batch, max_iter, tol, strideH);
  return hipGetLastError();
}

// qpb_factor_box for n <= 16: one launch of one wavefront, its first QP's lanes write the buffer
extern "C" hipError_t qpb_launch_gi_box_factor(int n, const double *H, double *bxfac, int32_t *fstatus,
                                               hipStream_t stream) {
  using qpb::box::BoxFactorOut;
  const auto kernel = n == 16 ? qpb::box::gi_box_kernel<true, false, BoxFactorOut>
                              : qpb::box::gi_box_kernel<false, false, BoxFactorOut>;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, stream, H, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr, nullptr, n, 1LL, 0, 0.0, BoxFactorOut{bxfac, fstatus});
  return hipGetLastError();
}

// qpb_solve_box_factored for n <= 16: the factored forms on such a buffer
extern "C" hipError_t qpb_launch_gi_box_factored(const qpb_desc *d, const double *bxfac, const double *f,
                                                 const double *lb, const double *ub, double *x, double *lam,
                                                 uint32_t *active, int32_t *status, int32_t *iters,
                                                 hipStream_t stream) {
  using qpb::box::BoxFactorIn;
  const long long blocks = (d->batch + qpb::box::QPB - 1) / qpb::box::QPB;
  const auto [max_iter, tol] = qpb_resolve_limits(d);
  const auto kernel = d->n == 16 ? qpb::box::gi_box_kernel<true, false, BoxFactorIn>
                                 : qpb::box::gi_box_kernel<false, false, BoxFactorIn>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64), 0, stream, bxfac, f, lb, ub, x, lam, active, status,
                     iters, d->n, (long long)d->batch, max_iter, tol, BoxFactorIn{bxfac});
  return hipGetLastError();
}
