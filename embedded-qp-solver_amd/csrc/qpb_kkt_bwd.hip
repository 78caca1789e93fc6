// qpb_kkt_bwd.hip -- the backward pass of a solve (qpb_solve_backward) for gfx950.
//
// Given a solved QP (x, lam, the active bit mask W of a linearly independent
// active set) and the cotangent g = dl/dx, the gradients of l with respect to
// H, f, A and b follow from ONE solve of the KKT system at fixed active set
//
//     [ H    A_W^T ] [ dx   ]     [ g ]
//     [ A_W   0    ] [ dlam ] = - [ 0 ]
//
//     dl/df = dx                        dl/dH   = 1/2 (dx x^T + x dx^T)
//     dl/db_i = -dlam_i                 dl/dA_i = dlam_i x^T + lam_i dx^T   (i in W, else 0)
//
// H is factored, the Schur complement A_W H^{-1} A_W^T is never formed (it
// squares the condition number): with H = L L^T, u = L^{-1} g and
// D_W = A_W L^{-T} (the forward kernels' D), the rows of D_W are
// orthogonalised in row order, D_W^T = Q R, and
//
//     z = -(u - Q Q^T u),   dx = L^{-T} z,   R dlam = -Q^T u.
//
// u is projected in two passes, z -= Q (Q^T z) twice with Q^T u the sum of the
// two coefficient vectors: the rounding of one pass, eps |u| inside span(Q),
// reaches dx through L^{-T} as eps cond(H) |g|, and A_W dx = 0 is lost at
// cond(H) = 1e10 when |W| is n or n - 1 (tests/test_bwd_cases.py).
//
// A row whose part orthogonal to the rows before it has |d2|^2 <= kDepTol |d|^2
// (the forward's dependency test) is skipped: dlam_i = 0, it keeps only the
// lam_i dx^T term of dl/dA_i.  The forward solve never produces such a mask.
//
// n <= 16, m <= 32 (kkt_bwd_dense_kernel): gi_dense's mapping, one QP per
// 16-lane DPP row, four per wavefront, in the LDS slot and with the shared
// steps of qpb_row16.h.  Lane l holds row l of H -> L and rows
// l, l + 16 of A -> D from the forward's right-looking sweep, which also
// carries u.  The orthogonalisation keeps every vector DISTRIBUTED (lane j
// holds component j): lane j keeps component j of every q_s in 16 statically
// indexed registers, a trip takes the owner's row through the exchange row in
// LDS, q_s . v is a row_sum per s and v -= sum_s c_s q_s is in-lane.  Two
// passes per row (classical Gram-Schmidt, repeated) give MGS-grade
// orthogonality with no dependence between the 16 products of a pass.  R's
// column t goes to LDS in the slot's layout (column-major, zero diagonal,
// 1 / R_tt in lane t), so both triangular solves are the lane-parallel
// DPP-fused back substitution (row16::back_subst_step).
#include "qpb_factor.h"  // the backward's buffer
#include "qpb_launch.h"  // with qpb.h
#include "qpb_row16.h"

namespace qpb {
namespace bwd {
using namespace row16;

// The QP's slot is qpb_row16.h's: L packed | R column-major with zero diagonal
// (the exchange row is its column 0).  After the solves the L part holds the
// vectors of the outer products.
constexpr int OFF_X = 0, OFF_DX = 16, OFF_DL = 32, OFF_LM = 64;  // x, dx | dlam, masked lam (32 each)
static_assert(OFF_LM + 32 <= L_SIZE, "the output vectors fit the dead L");

// p + q rounded once each and added: the value is symmetric under swapping the
// two products, so gH == gH^T bit for bit (a contracted fma(a, b, c d) is not)
__device__ __forceinline__ double sym2(double a, double b, double c, double d) {
#pragma clang fp contract(off)
  const double p = a * b;
  const double q = c * d;
  return p + q;
}

// What a form reads of a QP before its set-up.  The factor form (FM == 1) has
// no QP: nothing is loaded.  On a buffer (FM == 2, `fac`) whose H was not
// positive definite no QP counts as QPB_OK.
template <int FM>
__device__ __forceinline__ bool form_ok(const int32_t *statg, long long g, const double *fac) {
  if constexpr (FM == 1) return true;
  else if constexpr (FM == 2) return (statg ? statg[g] == QPB_OK : true) && fac[0] != (double)QPB_NOT_SPD;
  else return statg ? statg[g] == QPB_OK : true;
}
template <int FM>
__device__ __forceinline__ uint32_t form_mask(const uint32_t *actg, long long g) {
  if constexpr (FM == 1) return 0u;
  else return actg[g];
}
template <int FM>
__device__ __forceinline__ double form_gx(const double *gxg, long long e) {
  if constexpr (FM == 1) return 0.0;
  else return gxg[e];
}

// MR: rows of A per lane (m <= 16 MR).  N16: n == 16 (coalesced loads and
// stores through this QP's LDS slot); otherwise the rows are padded with the
// identity and padded variables take no part.
// SH (pass 1 of qpb_solve_shared_backward): H and / or A is one matrix for the
// whole batch, its QP stride 0; the QPB_SHARED_* bits ride in `m`, at kShShift.
constexpr int kShShift = 28;
static_assert(QPB_MAX_M < (1 << kShShift) && (3 << kShShift) > 0);
// FMP (empty, or Form<FM>): the forms around a backward factor buffer
// (qpb_factor.h, bfct).  FM == 1, qpb_factor_shared_backward's kernel: one
// workgroup runs this form's own load and sweep on the one H (Hg) and A (Ag)
// and its first row writes the buffer (gHg; the finding also to the int32 at
// gbg, which may be NULL) -- no QP is read.  FM == 2, qpb_solve_factored_backward:
// Hg is the buffer; L, 1 / L_kk, D and the multipliers of the u recursion are
// loaded and no sweep runs.  From the orthogonalisation on the code is one.
template <int FM>
using Form = std::integral_constant<int, FM>;
// GL (empty, or one const double *: the DU form, qpb_solve_backward_dual): the
// cotangent glam on the multipliers, B x m in lam's layout, as the lower
// right-hand side of the KKT system.  Its entries on the rows of W are
// scattered to the rows' positions (g), R^T w = g is solved on R's columns,
// Q w leaves z after the two projection passes and w joins the right-hand side
// of the R solve.  Deduced from the launch's trailing argument; the other
// forms have no such argument and none of this code.  On a buffer (FM == 2,
// qpb_solve_factored_backward_dual) the four steps are the same code behind the
// factored load: R and Q are per QP, from the orthogonalisation, either way.
// MU (qpb_solve_factored_backward_multi, both kernels, on a buffer only: FM ==
// 2, with and without glam): T right-hand sides per QP.  The pack's last
// argument, a Multi, which only this form has, carries T and the QP stride of
// the right-hand sides in directions (T, or 0 for one set that the whole batch
// reads).  Direction t of QP k reads gx + (k stride + t) n and glam +
// (k stride + t) m and writes gf + (k T + t) n and gb + (k T + t) m.  The
// factored load and the orthogonalisation run once -- neither reads gx -- and
// L, 1 / L_kk, Q, R and the rows' positions stay where they are; a loop over t
// takes u from the buffer's multipliers and repeats the rest of the
// single-direction form operation for operation, so every direction's bits are
// that form's.  x, lam, gH and gA are not arguments of the call: NULL, never read.
struct Multi {
  int T;
  long long stride;
};
// BX (qpb_solve_range_box_backward, both kernels, FM == 0, plain and SH, with and
// without glam): the rows are the mg rows of G and then the n variables' unit
// rows, m = mg + n in all -- the problem of qpb_solve_backward on A' = [G; I]
// with A' never in memory.  The pack's last argument, a Box, which only this
// form has, carries mg, the `lower` bit masks and the outputs that take gb's
// place.  Ag is G (QP stride mg n, unread at mg == 0); a row >= mg is made in
// registers where the other forms load it, and from the sweep on no operation
// differs, so L, D, Q, R, dx and dlam are that call's bits.  gAg is gG: the
// rows < mg.  An element of gb goes to the lower-side array where the row's
// `lower` bit is set and to the upper-side one otherwise, +0.0 to the other; gbw
// (pass 2's, else NULL) takes the rows < mg unrouted.  gbg is not read.
struct Box {
  int mg;
  const uint32_t *lower;          // ceil(m / 32) words per QP, or NULL: every row to the upper side
  double *gbl, *gbu, *glb, *gub;  // B x mg, B x mg, B x n, B x n; any may be NULL
  double *gbw;                    // B x mg
};
template <class... GL>
inline constexpr bool tail_is_multi = (std::is_same_v<GL, Multi> || ...);
template <class... GL>
inline constexpr bool tail_is_box = (std::is_same_v<GL, Box> || ...);
template <class... GL>
inline constexpr bool tail_ok = std::is_same_v<void(GL...), void()> || std::is_same_v<void(GL...), void(const double *)> ||
                                std::is_same_v<void(GL...), void(Multi)> ||
                                std::is_same_v<void(GL...), void(const double *, Multi)> ||
                                std::is_same_v<void(GL...), void(Box)> ||
                                std::is_same_v<void(GL...), void(const double *, Box)>;
__device__ __forceinline__ const double *tail_glam(const double *p) { return p; }
__device__ __forceinline__ const double *tail_glam(const double *p, Multi) { return p; }
__device__ __forceinline__ Multi tail_multi(Multi mu) { return mu; }
__device__ __forceinline__ Multi tail_multi(const double *, Multi mu) { return mu; }
__device__ __forceinline__ const double *tail_glam(const double *p, Box) { return p; }
__device__ __forceinline__ Box tail_box(Box bx) { return bx; }
__device__ __forceinline__ Box tail_box(const double *, Box bx) { return bx; }
// the routed pair of one element of gb: v to the side the row's `lower` bit names, +0.0 to the other
__device__ __forceinline__ void store_routed(double *lo, double *up, long long e, bool lower, double v) {
  if (lo) lo[e] = lower ? v : 0.0;
  if (up) up[e] = lower ? 0.0 : v;
}

template <int MR, bool N16, bool SH = false, class... FMP, class... GL>
__global__ __launch_bounds__(64, 3) void kkt_bwd_dense_kernel(
    const double *__restrict__ Hg, const double *__restrict__ Ag, const double *__restrict__ xg,
    const double *__restrict__ lamg, const uint32_t *__restrict__ actg, const int32_t *__restrict__ statg,
    const double *__restrict__ gxg, double *__restrict__ gHg, double *__restrict__ gfg, double *__restrict__ gAg,
    double *__restrict__ gbg, int n, int m, long long batch, GL... glamg) {
  constexpr int FM = (0 + ... + FMP::value);
  static_assert(sizeof...(FMP) <= 1 && FM >= 0 && FM <= 2 && !(SH && FM != 0), "one form at most, on its own strides");
  constexpr bool MU = tail_is_multi<GL...>;
  constexpr bool BX = tail_is_box<GL...>;
  constexpr bool DU = sizeof...(GL) - (MU ? 1 : 0) - (BX ? 1 : 0) == 1;
  static_assert(tail_ok<GL...> && !(DU && FM == 1) && !(MU && FM != 2) && !(BX && FM != 0),
                "glam is one array, beside H and A or a buffer of them; T directions on a buffer only; a box beside H and G only");
  __shared__ double lds[QPB * SLOT];
  [[maybe_unused]] int shared = 0;
  if constexpr (SH) {
    shared = m >> kShShift;
    m &= (1 << kShShift) - 1;
  }
  const int l = threadIdx.x & (NL - 1);
  const int slot = threadIdx.x >> 4;
  const long long g = ragged_qp(blockIdx.x, slot, batch).g;
  if constexpr (N16) n = NL;
  double *base = slot_base(lds, slot);
  double *Lp = base + OFF_L;
  double *R = base + OFF_R;
  double *xch = R;

  // ------------------------------------------------------------------ load
  const bool var = N16 || l < n;
  const int lc = var ? l : n - 1;
  const double *Hq = SH ? Hg + ((shared & QPB_SHARED_H) ? 0 : g) * (long long)n * n : Hg + g * (long long)n * n;
  // m == 0: the (masked) row loads read H
  [[maybe_unused]] int mg = m;  // BX: the rows of G, of the m = mg + n rows
  if constexpr (BX) mg = tail_box(glamg...).mg;
  const int ma = BX ? mg : m;  // the rows in memory at Ag
  const double *Aq =
      ma > 0 ? (SH ? Ag + ((shared & QPB_SHARED_A) ? 0 : g) * (long long)ma * n : Ag + g * (long long)ma * n) : Hq;
  // (FM == 2: nor does any QP on a buffer whose H was not positive definite)
  const bool ok = form_ok<FM>(statg, g, Hg);
  // a QP that is not QPB_OK takes no trips and stores zeros
  uint32_t W = (m > 0 && ok) ? form_mask<FM>(actg, g) : 0u;
  if (m < 32) W &= (1u << m) - 1u;
  double gv = 0.0;  // (MU: per direction, below)
  if constexpr (!MU) gv = form_gx<FM>(gxg, g * n + lc);
  [[maybe_unused]] double gl[MR];  // DU: glam of the lane's rows, 0 outside W (whatever it holds there)
  if constexpr (DU && !MU) {
    const double *__restrict__ glq = tail_glam(glamg...) + g * (long long)m;  // (the form has m > 0)
#pragma unroll
    for (int r = 0; r < MR; ++r) {
      const int row = l + NL * r;
      const double v = glq[row < m ? row : 0];
      gl[r] = ((W >> row) & 1u) ? v : 0.0;
    }
  }
  double Lr[NL];     // row l of H, becomes row l of L
  double E[MR][NL];  // rows l, l + 16 of A, become rows of D = A L^{-T}
  double ya, ul, invLd;
  if constexpr (FM == 2) {
    ya = var ? gv : 0.0, ul = 0.0;
    // The buffer in place of H and A: every load is 16 bytes per lane at
    // consecutive addresses over the QP's lanes, the same for the wave's four
    // QPs.  L goes straight to the slot.
    constexpr bfct::Layout y = bfct::layout(NL, NL * MR);
    const double *fac = Hg;
#pragma unroll
    for (int t = 0; t < bfct::kDenseL / (2 * NL); ++t) {
      const double2 v = *reinterpret_cast<const double2 *>(&fac[y.L + (t * NL + l) * 2]);
      if ((t * NL + l) * 2 < L_SIZE) *reinterpret_cast<double2 *>(&Lp[(t * NL + l) * 2]) = v;
    }
    invLd = fac[y.ik + l];
    if constexpr (!MU) {  // (MU takes every direction's u behind the orthogonalisation; the block keeps its indentation)
    double nc[NL];
#pragma unroll
    for (int t = 0; t < NL / 2; ++t) {
      const double2 v = *reinterpret_cast<const double2 *>(&fac[y.nc + (t * NL + l) * 2]);
      nc[2 * t] = v.x;
      nc[2 * t + 1] = v.y;
    }
    // u = L^{-1} g from the sweep's multipliers in the sweep's order and with
    // its instruction: u_k = g_k / L_kk is taken on lane k at step k (there
    // the lane's own 1 / L_ll is the step's), then g += g_k nc_k.  The FMA
    // reads the g it wrote the step before: the hazard's wait states each time.
    unroll<NL>([&](auto K) {
      constexpr int k = K;
      ul = l == k ? ya * invLd : ul;
      pin(ul);  // (as in the sweep: the select would sink with every step's g alive)
      fmac_bc_nop<k>(ya, ya, nc[k]);
    });
    // (D after u: the multipliers are dead by then, and nothing may hoist the
    // loads above it -- the 32 registers of nc beside the 64 of D spill)
    __builtin_amdgcn_sched_barrier(0);
    }  // !MU
#pragma unroll
    for (int r = 0; r < MR; ++r)
#pragma unroll
      for (int t = 0; t < NL / 2; ++t) {
        const double2 v = *reinterpret_cast<const double2 *>(&fac[y.D + ((r * (NL / 2) + t) * NL + l) * 2]);
        E[r][2 * t] = v.x;
        E[r][2 * t + 1] = v.y;
      }
    wave_lds_sync();
  } else {  // (the unfactored load and sweep keep their indentation, down to "FM != 2")
  if constexpr (N16) {
    // coalesced 16-byte loads, two whole rows of each of the wave's 4 QPs per
    // instruction; the rows reach their owner lanes through a transpose in
    // this QP's LDS slot (qpb_gi.hip)
    const int hr = l >> 3, hc = 2 * (l & 7);
    auto stage = [&](const double2(&v)[8]) {
      wave_lds_sync();
#pragma unroll
      for (int t = 0; t < 8; ++t) *reinterpret_cast<double2 *>(&base[(2 * t + hr) * RS + hc]) = v[t];
      wave_lds_sync();
    };
    double2 hv[8], av[MR][8];
#pragma unroll
    for (int t = 0; t < 8; ++t) hv[t] = *reinterpret_cast<const double2 *>(&Hq[(2 * t + hr) * NL + hc]);
#pragma unroll
    for (int r = 0; r < MR; ++r)
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        // rows past m read a valid row (m == 0: of H) and are zeroed: no branch around a load
        const int row = NL * r + 2 * t + hr;
        const double2 a = *reinterpret_cast<const double2 *>(&Aq[(row < ma ? row : 0) * NL + hc]);
        asm volatile("" ::"v"(a.x), "v"(a.y));
        if constexpr (BX) {
          // a row >= mg is variable row - mg's unit row, made here in place of the load (selected per
          // component: a select between two double2 objects goes through their addresses, and the
          // staging arrays then live in scratch)
          const int j = row - mg;
          const double u0 = (row < m && j == hc) ? 1.0 : 0.0, u1 = (row < m && j == hc + 1) ? 1.0 : 0.0;
          av[r][t] = make_double2(row < mg ? a.x : u0, row < mg ? a.y : u1);
        } else {
          av[r][t] = row < m ? a : make_double2(0.0, 0.0);
        }
      }
    stage(hv);
    lds_row16(&base[l * RS], Lr);
#pragma unroll
    for (int r = 0; r < MR; ++r) {
      stage(av[r]);
      lds_row16(&base[l * RS], E[r]);
    }
    wave_lds_sync();
  } else {
#pragma unroll
    for (int j = 0; j < NL; ++j) Lr[j] = h_padded(Hq, l, lc, n, j);
#pragma unroll
    for (int r = 0; r < MR; ++r) {
      const int row = l + NL * r;
      const bool rok = row < ma;
      const int rc = rok ? row : 0;
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const double a = Aq[rc * n + (j < n ? j : n - 1)];
        if constexpr (BX) E[r][j] = (rok && j < n) ? a : (row >= mg && row < m && j == row - mg) ? 1.0 : 0.0;
        else E[r][j] = (rok && j < n) ? a : 0.0;
      }
    }
  }

  // ---- H = L L^T, D = A L^{-T}, u = L^{-1} g: the forward's right-looking
  // sweep (qpb_gi.hip).  Step k: the pivot row is read straight from lane k by
  // the DPP-fused FMAs; the sched_barrier and the rsq chain keep every write
  // of Lr[j] and of the running g (previous step) well over two instructions
  // before these reads.  u_k = g_k / L_kk is final at step k, on lane k.
  // D's update takes a_jk from lane j (column k of ITS row, the entry that
  // becomes L_jk), not a_kj from the pivot row: the two triangles of the
  // trailing block agree to eps |H| only, which next to a pivot of 1e-10 |H| is
  // another L -- and D from one L with u and dx from the other broke both
  // certificates at cond(H) = 1e10 (1e-9 where the wave kernel has 1e-15).
  ya = var ? gv : 0.0, ul = 0.0, invLd = 0.0;
  [[maybe_unused]] bool spd = true;               // FM == 1: every pivot was a positive finite number
  unroll<NL>([&](auto K) {
    constexpr int k = K;
    __builtin_amdgcn_sched_barrier(0);
    const double akk = bc<k>(Lr[k]);
    const double ik = rsq1(akk);
    const double ik2 = ik * ik;
    const double nc = -(Lr[k] * ik2);
    if constexpr (FM == 1) {
      // the lane's multiplier of the step, to its place in the buffer
      if (slot == 0) gHg[bfct::layout(NL, NL * MR).nc + ((k / 2) * NL + l) * 2 + (k & 1)] = nc;
      spd = spd && akk > 0.0 && akk < kInf;
    }
    double ne2[MR];
#pragma unroll
    for (int r = 0; r < MR; ++r) {
      const double e = E[r][k];
      ne2[r] = -(e * ik2);
      E[r][k] = e * ik;
      pin(E[r][k]);
    }
    // (pinned: the selects would otherwise sink past the sweep with all 16 steps' operands alive)
    ul = l == k ? ya * ik : ul;
    invLd = l == k ? ik : invLd;
    pin(ul);
    pin(invLd);
    unroll<NL - 1 - k>([&](auto J) {
      constexpr int j = k + 1 + J;
#pragma unroll
      for (int r = 0; r < MR; ++r) fmac_bc<j>(E[r][j], Lr[k], ne2[r]);  // a_jk of lane j: L's own entry
      fmac_bc<k>(Lr[j], Lr[j], nc);
    });
    fmac_bc<k>(ya, ya, nc);  // lane k's own g_k becomes 0 (dead)
    Lr[k] *= ik;
    pin(Lr[k]);
  });
  __builtin_amdgcn_sched_barrier(0);
  store_l(Lp, l, Lr);  // for the last solve
  if constexpr (FM == 1) {
    // ---- the factor kernel ends here: the first row writes the buffer, L as
    // the slot holds it
    wave_lds_sync();
    if (slot == 0) {
      constexpr bfct::Layout y = bfct::layout(NL, NL * MR);
      double *fac = gHg;
      const int found = spd ? QPB_OK : QPB_NOT_SPD;
      if (l < bfct::kHdr) fac[l] = l == 0 ? (double)found : l == 1 ? (double)n : l == 2 ? (double)m : l == 3 ? 16.0 : 0.0;
      if (l == 0 && gbg) *reinterpret_cast<int32_t *>(gbg) = found;
#pragma unroll
      for (int t = 0; t < bfct::kDenseL / (2 * NL); ++t) {
        const int e = (t * NL + l) * 2;
        *reinterpret_cast<double2 *>(&fac[y.L + e]) =
            e < L_SIZE ? *reinterpret_cast<const double2 *>(&Lp[e]) : make_double2(0.0, 0.0);
      }
      fac[y.ik + l] = invLd;
#pragma unroll
      for (int r = 0; r < MR; ++r)
#pragma unroll
        for (int t = 0; t < NL / 2; ++t)
          *reinterpret_cast<double2 *>(&fac[y.D + ((r * (NL / 2) + t) * NL + l) * 2]) =
              make_double2(E[r][2 * t], E[r][2 * t + 1]);
    }
    return;
  }
  }  // FM != 2
  // R zeroed in pairs at lane-rotated positions (qpb_gi_box.hip)
#pragma unroll
  for (int j = 0; j < NL; j += 2)
    *reinterpret_cast<double2 *>(&R[l * NL + ((j + 2 * l) & (NL - 1))]) = make_double2(0.0, 0.0);

  // ------------------------------------------------ D_W^T = Q R, row order
  double Qt[NL];  // component l of q_0 .. q_15 (0 past cnt)
#pragma unroll
  for (int s = 0; s < NL; ++s) Qt[s] = 0.0;
  int cnt = 0;         // independent rows so far = the next position
  double invRd = 0.0;  // 1 / R[l][l]
  int pos[MR];         // position of the lane's rows, -1: not in W or skipped
#pragma unroll
  for (int r = 0; r < MR; ++r) pos[r] = -1;
  uint32_t rem = W;
  // v -= sum_s (q_s . v) q_s over the positions in use by any of the wave's
  // QPs; a QP's unused q_s are 0 and change nothing.  cl += (q_l . v).
  auto project = [&](double &v, double &cl, int smax) {
    const double v0 = v;
    unroll<NL>([&](auto S) {
      constexpr int s = S;
      if (s < smax) {
        const double c = row_sum(Qt[s] * v0);
        cl += (l == s) ? c : 0.0;
        v = __builtin_fma(-c, Qt[s], v);
      }
    });
  };
  while (wave_any(rem != 0u)) {
    const bool valid = rem != 0u;
    const int i = valid ? __builtin_ctz(rem) : 0;
    rem &= rem - 1u;
    const int owner = i & (NL - 1);
    wave_lds_sync();
    if (valid && l == owner) {
#pragma unroll
      for (int j = 0; j < NL; j += 2) {
        double a = E[0][j], b = E[0][j + 1];
        if constexpr (MR > 1) {
          a = i >= NL ? E[1][j] : a;
          b = i >= NL ? E[1][j + 1] : b;
        }
        *reinterpret_cast<double2 *>(&xch[j]) = make_double2(a, b);
      }
    }
    wave_lds_sync();
    double v = valid ? xch[l] : 0.0;
    const int smax = wave_max4(cnt);
    const double dd = row_sum(v * v);  // |d|^2
    double cl = 0.0;                   // R[l][cnt]
    project(v, cl, smax);
    project(v, cl, smax);
    const double nd2 = row_sum(v * v);  // |d2|^2
    const bool indep = valid && cnt < NL && nd2 > kDepTol * dd;
    const double rn = rsq(nd2);
    if (indep) {
      const double ql = v * rn;
      unroll<NL>([&](auto S) {
        constexpr int s = S;
        Qt[s] = cnt == s ? ql : Qt[s];
      });
      if (cnt > 0) R[cnt * NL + l] = cl;  // column 0 has no entry above the diagonal
      invRd = l == cnt ? rn : invRd;
      if (l == owner) {
        if (i < NL) pos[0] = cnt;
        if constexpr (MR > 1)
          if (i >= NL) pos[1] = cnt;
      }
      ++cnt;
    }
  }
  wave_lds_sync();

  // ---- z = -(u - Q Q^T u), R dlam = -Q^T u
  const int qmax = wave_max4(cnt);
  if constexpr (MU) {
    // ---- T directions on the one load and orthogonalisation.  Per direction:
    // the multipliers again from the buffer (hot in cache; D's registers are
    // dead by now), the u recursion of the factored load, and the statements
    // below from the two projection passes to the stores of gf and gb.
    const Multi mu = tail_multi(glamg...);
    constexpr bfct::Layout fy = bfct::layout(NL, NL * MR);
    const double *__restrict__ fac = Hg;
    const bool lives = ragged_qp(blockIdx.x, slot, batch).live;
    const double *__restrict__ gq = gxg + g * mu.stride * n + lc;
    [[maybe_unused]] const double *__restrict__ glq = nullptr;
    if constexpr (DU) glq = tail_glam(glamg...) + g * mu.stride * m;  // (the form has m > 0)
    for (int t = 0; t < mu.T; ++t) {
      const double gt = gq[(long long)t * n];
      [[maybe_unused]] double glt[MR];  // glam of the lane's rows, 0 outside W (whatever it holds there)
      if constexpr (DU) {
#pragma unroll
        for (int r = 0; r < MR; ++r) {
          const int row = l + NL * r;
          const double v = glq[(long long)t * m + (row < m ? row : 0)];
          glt[r] = ((W >> row) & 1u) ? v : 0.0;
        }
      }
      double yt = var ? gt : 0.0, ut = 0.0;
      {
        double nc[NL];
#pragma unroll
        for (int h = 0; h < NL / 2; ++h) {
          const double2 v = *reinterpret_cast<const double2 *>(&fac[fy.nc + (h * NL + l) * 2]);
          nc[2 * h] = v.x;
          nc[2 * h + 1] = v.y;
        }
        unroll<NL>([&](auto K) {
          constexpr int k = K;
          ut = l == k ? yt * invLd : ut;
          pin(ut);
          fmac_bc_nop<k>(yt, yt, nc[k]);
        });
      }
      double z = ut, cu = 0.0;
      project(z, cu, qmax);
      project(z, cu, qmax);
      z = -z;
      if constexpr (DU) {
        wave_lds_sync();
        xch[l] = 0.0;
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < MR; ++r)
          if (pos[r] >= 0) xch[pos[r]] = glt[r];
        wave_lds_sync();
        double w = xch[l];
        double Rc[NL];
        lds_row16(&R[l * NL], Rc);
        wave_lds_sync();
        {
          const double ninv = -invRd;
          unroll<NL - 1>([&](auto S) {
            constexpr int s = S;
            if (s + 1 < qmax) fmac_bc_nop<s>(w, w * ninv, l > s ? Rc[s] : 0.0);
          });
        }
        w *= invRd;
        {
          double nw = -w;
          pin(nw);
          dpp_ready(nw);
          unroll<NL>([&](auto S) {
            constexpr int s = S;
            if (s < qmax) fmac_bc<s>(z, nw, Qt[s]);
          });
        }
        cu -= w;
      }
      double y;  // dlam of position l
      {
        const double ninv = -invRd;
        double nacc = -cu;
        unroll<NL>([&](auto JJ) { back_subst_step<NL - 1 - JJ>(R, l, qmax, nacc, ninv); });
        y = nacc * invRd;
      }
      double dx;
      {
        const double ninv = -invLd;
        double nacc = z;
        unroll<NL>([&](auto JJ) {
          constexpr int j = NL - 1 - JJ;
          if (j > 0) {
            const double lj = l < j ? Lp[lrow(j) + l] : 0.0;
            fmac_bc_nop<j>(nacc, nacc * ninv, lj);
          }
        });
        dx = nacc * invLd;
      }
      wave_lds_sync();
      xch[l] = y;
      wave_lds_sync();
      double dl[MR];
#pragma unroll
      for (int r = 0; r < MR; ++r) dl[r] = pos[r] >= 0 ? xch[pos[r]] : 0.0;
      wave_lds_sync();
      if (!ok) dx = 0.0;
      const long long qt = g * (long long)mu.T + t;
      if (gfg && lives && var) gfg[qt * n + l] = dx;
#pragma unroll
      for (int r = 0; r < MR; ++r) {
        const int row = l + NL * r;
        if (gbg && lives && row < m) gbg[qt * m + row] = pos[r] >= 0 ? -dl[r] : 0.0;
      }
    }
    return;
  }
  // (u is projected twice as the rows are: one pass leaves eps |u| of it in the
  // span of Q, which L^{-T} magnifies by up to sqrt(cond H) -- all there is of
  // dx when W leaves little or no freedom; cu sums the two passes' Q^T z)
  double z = ul, cu = 0.0;
  project(z, cu, qmax);
  project(z, cu, qmax);
  z = -z;
  if constexpr (DU) {
    // ---- g: glam of the kept rows at their positions, through the exchange
    // row (0 past cnt; a skipped row has no position and its glam goes nowhere)
    wave_lds_sync();
    xch[l] = 0.0;
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < MR; ++r)
      if (pos[r] >= 0) xch[pos[r]] = gl[r];
    wave_lds_sync();
    double w = xch[l];
    // ---- R^T w = g, column-oriented: lane t holds column t of R above the
    // diagonal (the slot's layout), step s takes the finished w_s from lane s
    // and the lanes behind it subtract R[s][t] w_s.  1 / R_tt is 0 past cnt.
    double Rc[NL];
    lds_row16(&R[l * NL], Rc);
    wave_lds_sync();
    // The product is read from lane s by the FMA itself, as in
    // back_subst_step: it was written just before, so fmac_bc_nop issues the
    // DPP read hazard's wait states.
    {
      const double ninv = -invRd;
      unroll<NL - 1>([&](auto S) {
        constexpr int s = S;
        if (s + 1 < qmax) fmac_bc_nop<s>(w, w * ninv, l > s ? Rc[s] : 0.0);
      });
    }
    w *= invRd;
    // ---- z -= Q w, in-lane on the lane's components of the q_s (w_s from lane
    // s, fused); cu -= w makes the right-hand side of the R solve below
    // -Q^T u + w
    {
      // (pinned: left as -w, the compiler reassembles the pair from w's low
      // word and the flipped high word in front of every other FMA, inside
      // the hazard's window)
      double nw = -w;
      pin(nw);
      dpp_ready(nw);
      unroll<NL>([&](auto S) {
        constexpr int s = S;
        if (s < qmax) fmac_bc<s>(z, nw, Qt[s]);
      });
    }
    cu -= w;
  }
  double y;  // dlam of position l
  {
    const double ninv = -invRd;
    double nacc = -cu;
    unroll<NL>([&](auto JJ) { back_subst_step<NL - 1 - JJ>(R, l, qmax, nacc, ninv); });
    y = nacc * invRd;
  }
  // ---- L^T dx = z, the same back substitution on L's rows
  double dx;
  {
    const double ninv = -invLd;
    double nacc = z;
    unroll<NL>([&](auto JJ) {
      constexpr int j = NL - 1 - JJ;
      if (j > 0) {
        const double lj = l < j ? Lp[lrow(j) + l] : 0.0;
        fmac_bc_nop<j>(nacc, nacc * ninv, lj);
      }
    });
    dx = nacc * invLd;
  }
  // dlam to the rows' owners through the exchange row
  wave_lds_sync();
  xch[l] = y;
  wave_lds_sync();
  double dl[MR];
#pragma unroll
  for (int r = 0; r < MR; ++r) dl[r] = pos[r] >= 0 ? xch[pos[r]] : 0.0;
  wave_lds_sync();

  // ------------------------------------------------------------------ store
  // The lane's indices are formed again from an opaque copy of the thread id:
  // shared with the load phase, the address offsets would stay alive (spilled
  // to scratch) across the whole kernel.  x and lam are read here for the same
  // reason; the loads fly under the vector exchange below.
  unsigned tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int ls = tid & (NL - 1);
  const auto [lives, gs] = ragged_qp(blockIdx.x, tid >> 4, batch);
  const bool vars = N16 || ls < n;
  const double xv = xg[gs * n + (vars ? ls : n - 1)];
  double lmv[MR];  // lam of the lane's rows, 0 outside W
#pragma unroll
  for (int r = 0; r < MR; ++r) {
    const int row = ls + NL * r;
    const double lv = m > 0 ? lamg[gs * m + (row < m ? row : 0)] : 0.0;
    lmv[r] = ((W >> row) & 1u) ? lv : 0.0;
  }
  if (!ok) dx = 0.0;
  const double xo = (ok && vars) ? xv : 0.0;
  if (gfg && lives && vars) gfg[gs * n + ls] = dx;
#pragma unroll
  for (int r = 0; r < MR; ++r) {
    const int row = ls + NL * r;
    if constexpr (BX) {
      // (the class has m <= 32: one word of `lower`)
      const Box bx = tail_box(glamg...);
      const double v = pos[r] >= 0 ? -dl[r] : 0.0;
      if (lives && row < m) {
        const bool lo = bx.lower ? (bx.lower[gs] >> row) & 1u : false;
        if (row < mg) {
          store_routed(bx.gbl, bx.gbu, gs * mg + row, lo, v);
          if (bx.gbw) bx.gbw[gs * mg + row] = v;
        } else {
          store_routed(bx.glb, bx.gub, gs * n + (row - mg), lo, v);
        }
      }
    } else {
      if (gbg && lives && row < m) gbg[gs * m + row] = pos[r] >= 0 ? -dl[r] : 0.0;
    }
  }
  const bool wantA = gAg && ma > 0;
  if (!gHg && !wantA) return;  // wave-uniform
  // the vectors of the outer products, over the dead L
  base[OFF_X + ls] = xo;
  base[OFF_DX + ls] = dx;
#pragma unroll
  for (int r = 0; r < MR; ++r) {
    base[OFF_DL + ls + NL * r] = dl[r];
    base[OFF_LM + ls + NL * r] = lmv[r];
  }
  wave_lds_sync();
  const double *X = base + OFF_X, *DX = base + OFF_DX, *DL = base + OFF_DL, *LM = base + OFF_LM;
  if constexpr (N16) {
    // lane l writes columns 2 (l & 7), +1 of rows 2 t + (l >> 3): 256 contiguous bytes per QP and store
    const int hr = ls >> 3, hc = 2 * (ls & 7);
    const double x0 = X[hc], x1 = X[hc + 1], d0 = DX[hc], d1 = DX[hc + 1];
    if (gHg && lives) {
      double *o = gHg + gs * (long long)(NL * NL);
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int row = 2 * t + hr;
        const double dr = DX[row], xr = X[row];
        *reinterpret_cast<double2 *>(&o[row * NL + hc]) =
            make_double2(0.5 * sym2(dr, x0, xr, d0), 0.5 * sym2(dr, x1, xr, d1));
      }
    }
    if (wantA && lives) {
      double *o = gAg + gs * (long long)ma * NL;
#pragma unroll
      for (int r = 0; r < MR; ++r)
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int row = NL * r + 2 * t + hr;
          if (row < ma) {
            const double dr = DL[row], lr = LM[row];
            *reinterpret_cast<double2 *>(&o[row * NL + hc]) =
                make_double2(sym2(dr, x0, lr, d0), sym2(dr, x1, lr, d1));
          }
        }
    }
  } else {
    // element e of the row-major output at lane e mod 16
    if (gHg && lives) {
      double *o = gHg + gs * (long long)n * n;
      for (int e = ls; e < n * n; e += NL) {
        const int row = e / n, col = e - row * n;
        o[e] = 0.5 * sym2(DX[row], X[col], X[row], DX[col]);
      }
    }
    if (wantA && lives) {
      double *o = gAg + gs * (long long)ma * n;
      for (int e = ls; e < ma * n; e += NL) {
        const int row = e / n, col = e - row * n;
        o[e] = sym2(DL[row], X[col], LM[row], DX[col]);
      }
    }
  }
}

// ---- 16 < n <= 32 or 32 < m <= 64: one QP per wavefront ----------------------
// The matrices live in LDS in gi_wave's manner: L in the lower triangle of a
// 32 x 33 block (odd stride: rows and columns are both conflict-free), R above
// its diagonal, the orthonormal rows q_s in a second block.  Lane j < 32 holds
// component j of the running vectors; a QP is alone in its wave, so every
// loop bound is wave-uniform.  The algebra is the dense kernel's: row i of
// D_W = A_W L^{-T} comes from a forward substitution as it is met, in row
// order, and is orthogonalised against the q_s before it in two passes.
// H is padded to 32 x 32 with the identity and the unused q_s are zero, so the
// loops over components and positions have constant bounds and unroll: their
// LDS reads issue back to back instead of one per loop trip.
constexpr int WN = 32;       // variables (lanes that carry a component)
constexpr int WS = WN + 1;   // row stride
constexpr int W_L = 0, W_Q = WN * WS, W_V = 2 * WN * WS;  // L (+ R) | Q | vectors
// vectors: v, c, u | 1 / R_tt | position of a row (64) | x, dx | dlam, masked lam (64 each)
constexpr int W_C = W_V + 32, W_U = W_C + 32, W_IR = W_U + 32, W_POS = W_IR + 32, W_X = W_POS + 64,
              W_DX = W_X + 32, W_DL = W_DX + 32, W_LM = W_DL + 64, W_SIZE = W_LM + 64;
constexpr int W_COL = WN + 2;  // the pivot column of a factorisation step, zero past the matrix
static_assert((W_SIZE + W_COL) * 8 <= 20480, "8 waves per CU by LDS");

// sum over the 64 lanes, the same bits on every lane
__device__ __forceinline__ double wave_sum(double t) {
  t = row_sum(t);
  return (readlane_d(t, 0) + readlane_d(t, 16)) + (readlane_d(t, 32) + readlane_d(t, 48));
}

// FMP: the dense kernel's forms around a backward factor buffer.  FM == 1 runs
// the factorisation on the one H and the forward substitution for all m rows
// of the one A, and writes the buffer (gHg, the finding also to the int32 at
// gbg); FM == 2 (Hg is the buffer) copies L's image into LDS, takes u from the
// stored L and 1 / L_kk by the operations of the factorisation loop, and an
// active row's v is one load.
// GL: the dense kernel's DU form.  Lane r < m holds glam of row r; g goes to
// the rows' positions through vb, R^T w = g runs on R above L's diagonal as the
// R solve does, and Q w leaves z through cb, by the loop of a projection pass.
template <bool SH = false, class... FMP, class... GL>
__global__ __launch_bounds__(64) void kkt_bwd_wave_kernel(
    const double *__restrict__ Hg, const double *__restrict__ Ag, const double *__restrict__ xg,
    const double *__restrict__ lamg, const uint32_t *__restrict__ actg, const int32_t *__restrict__ statg,
    const double *__restrict__ gxg, double *__restrict__ gHg, double *__restrict__ gfg, double *__restrict__ gAg,
    double *__restrict__ gbg, int n, int m, long long batch, GL... glamg) {
  constexpr int FM = (0 + ... + FMP::value);
  static_assert(sizeof...(FMP) <= 1 && FM >= 0 && FM <= 2 && !(SH && FM != 0), "one form at most, on its own strides");
  constexpr bool MU = tail_is_multi<GL...>;
  constexpr bool BX = tail_is_box<GL...>;
  constexpr bool DU = sizeof...(GL) - (MU ? 1 : 0) - (BX ? 1 : 0) == 1;
  static_assert(tail_ok<GL...> && !(DU && FM == 1) && !(MU && FM != 2) && !(BX && FM != 0),
                "glam is one array, beside H and A or a buffer of them; T directions on a buffer only; a box beside H and G only");
  __shared__ double lds[W_SIZE];
  // an object of its own: the factorisation's trailing update reads it while
  // it writes L, and the compiler can then batch the reads of an unrolled trip
  __shared__ double colk[W_COL];
  [[maybe_unused]] int shared = 0;
  if constexpr (SH) {
    shared = m >> kShShift;
    m &= (1 << kShShift) - 1;
  }
  const int lane = threadIdx.x;
  const int i = lane & (WN - 1), half = lane >> 5;
  const bool low = lane < WN;      // the lanes that carry a component
  const long long g = blockIdx.x;  // one workgroup of one wave per QP: always < batch
  double *Lm = lds + W_L, *Qm = lds + W_Q;
  double *vb = lds + W_V, *cb = lds + W_C, *ub = lds + W_U, *ir = lds + W_IR, *posb = lds + W_POS;
  const double *Hq = SH ? Hg + ((shared & QPB_SHARED_H) ? 0 : g) * (long long)n * n : Hg + g * (long long)n * n;
  [[maybe_unused]] int mg = m;  // BX: the rows of G, of the m = mg + n rows
  if constexpr (BX) mg = tail_box(glamg...).mg;
  const int ma = BX ? mg : m;  // the rows in memory at Ag (BX, mg == 0: Ag is never read)
  const double *Aq = SH ? Ag + ((shared & QPB_SHARED_A) ? 0 : g) * (long long)ma * n : Ag + g * (long long)ma * n;
  const bool ok = form_ok<FM>(statg, g, Hg);
  // the active mask as one 64-bit word (wave-uniform); a QP that is not QPB_OK takes no trips
  const int words = (m + 31) / 32;
  unsigned long long W = 0;
  if (FM != 1 && ok && m > 0) {
    W = actg[g * words];
    if (words > 1) W |= (unsigned long long)actg[g * words + 1] << 32;
    if (m < 64) W &= (1ull << m) - 1ull;
  }
  W = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(W >> 32)) << 32) |
      (unsigned)__builtin_amdgcn_readfirstlane((int)W);
  [[maybe_unused]] double glv = 0.0;  // DU: glam of row `lane`, 0 outside W (whatever it holds there)
  if constexpr (DU && !MU) {
    const double v = tail_glam(glamg...)[g * m + (lane < m ? lane : 0)];  // (the form has m > 0)
    glv = ((W >> lane) & 1ull) ? v : 0.0;
  }
  [[maybe_unused]] const bfct::Layout fy = bfct::layout(FM != 0 ? n : 17, m);  // the wave class's offsets
  if constexpr (FM == 2) {
    // L's image as the factor kernel left it, Q zero
    static_assert(W_L == 0 && bfct::kWaveL == WN * WS && bfct::kWaveL % 2 == 0);
    for (int e = lane; e < bfct::kWaveL / 2; e += 64) {
      const double2 v = *reinterpret_cast<const double2 *>(&Hg[fy.L + 2 * e]);
      Lm[2 * e] = v.x;
      Lm[2 * e + 1] = v.y;
    }
    for (int e = lane; e < WN * WN; e += 64) Qm[(e >> 5) * WS + (e & (WN - 1))] = 0.0;
  } else {  // (the unfactored load keeps its indentation)
  // H padded with the identity, Q zero
  for (int e = lane; e < WN * WN; e += 64) {
    const int row = e >> 5, col = e & (WN - 1);
    const bool in = row < n && col < n;
    const double h = Hq[in ? row * n + col : 0];
    Lm[row * WS + col] = in ? h : (row == col ? 1.0 : 0.0);
    Qm[row * WS + col] = 0.0;
  }
  }
  posb[lane] = -1.0;
  if (lane < W_COL) colk[lane] = 0.0;
  const bool var = lane < n;
  double ui = 0.0;  // the running g, u_k = (L^{-1} g)_k from step k on (MU: per direction, below)
  if constexpr (!MU) ui = var ? form_gx<FM>(gxg, g * n + lane) : 0.0;
  double invLd = var ? 0.0 : 1.0;                           // 1 / L[lane][lane] (1 on the padding)
  if constexpr (FM == 2) invLd = low ? Hg[fy.ik + lane] : 1.0;
  wave_lds_sync();
  [[maybe_unused]] bool spd = true;  // FM == 1: every pivot was a positive finite number

  // ---- H = L L^T (right-looking, in place) and u = L^{-1} g.  Step k updates
  // the whole rows k+1.. of the symmetric trailing block, the two halves of
  // the wave on alternate columns (the upper triangle is redundant and free:
  // no predicate in the loop; the last trip of the upper half may touch the
  // row's padding word, colk is zero there)
  if constexpr (MU) {
    // (every direction's u behind the orthogonalisation, by the loop below)
  } else if constexpr (FM == 2) {
    // u alone, by the loop's own operations on the stored L and 1 / L_kk
    for (int k = 0; k < n; ++k) {
      const double uk = readlane_d(ui, k) * readlane_d(invLd, k);
      const double lik = (low && lane > k) ? Lm[i * WS + k] : 0.0;
      if (lane == k) ui = uk;
      else if (low && lane > k) ui = __builtin_fma(-lik, uk, ui);
    }
  } else  // (the factorisation loop keeps its indentation)
  for (int k = 0; k < n; ++k) {
    if constexpr (FM == 1) {
      const double akk = Lm[k * WS + k];
      spd = spd && akk > 0.0 && akk < kInf;
    }
    const double ik = rsq(Lm[k * WS + k]);
    const double uk = readlane_d(ui, k) * ik;
    const double lik = i >= k ? Lm[i * WS + k] * ik : 0.0;
    wave_lds_sync();
    if (half == 0) {
      colk[i] = i > k ? lik : 0.0;
      if (i >= k) Lm[i * WS + k] = lik;
    }
    if (lane == k) {
      ui = uk;
      invLd = ik;
    } else if (low && lane > k) {
      ui = __builtin_fma(-lik, uk, ui);
    }
    wave_lds_sync();
    const double nl = i > k ? -lik : 0.0;
    double *row = Lm + i * WS + k + 1 + half;
    const double *col = colk + k + 1 + half;
    const int trips = (WN - k) / 2;
#pragma unroll 4
    for (int jj = 0; jj < trips; ++jj) row[2 * jj] = __builtin_fma(nl, col[2 * jj], row[2 * jj]);
    wave_lds_sync();
  }
  if constexpr (FM == 1) {
    // ---- the factor kernel ends here: every row of D, L's image, the buffer
    double *fac = gHg;
    const int found = spd ? QPB_OK : QPB_NOT_SPD;
    if (lane < bfct::kHdr)
      fac[lane] = lane == 0 ? (double)found : lane == 1 ? (double)n : lane == 2 ? (double)m : lane == 3 ? 32.0 : 0.0;
    if (lane == 0 && gbg) *reinterpret_cast<int32_t *>(gbg) = found;
    // (a row's padding word is never initialised in LDS and never read: zero in the buffer)
    for (int e = lane; e < bfct::kWaveL; e += 64) fac[fy.L + e] = e % WS == WN ? 0.0 : Lm[e];
    if (low) fac[fy.ik + lane] = invLd;
    for (int r = 0; r < m; ++r) {
      // (the loop of an active row below, for every row)
      double v = var ? Aq[r * n + lane] : 0.0;
#pragma unroll
      for (int k = 0; k < WN; ++k) {
        const double dk = readlane_d(v * invLd, k);
        const double lk = (low && lane > k) ? Lm[i * WS + k] : 0.0;
        v = lane == k ? dk : __builtin_fma(-lk, dk, v);
      }
      if (low) fac[fy.D + r * WN + lane] = v;
    }
    return;
  }
  if (low) ub[lane] = ui;
  wave_lds_sync();

  // ---- D_W^T = Q R over the active rows in row order
  // c_lane = q_lane . v and v -= sum_s c_s q_s over the rows so far (the q_s
  // past them are zero); cl += c_lane
  int cnt = 0;
  auto project = [&](double &v, double &cl) {
    wave_lds_sync();
    if (low) vb[lane] = v;
    wave_lds_sync();
    if (low) {
      double c0 = 0.0, c1 = 0.0;
#pragma unroll
      for (int j = 0; j < WN; j += 2) {
        c0 = __builtin_fma(Qm[lane * WS + j], vb[j], c0);
        c1 = __builtin_fma(Qm[lane * WS + j + 1], vb[j + 1], c1);
      }
      const double c = c0 + c1;
      cl += c;
      cb[lane] = c;
    }
    wave_lds_sync();
    if (low) {
      for (int s0 = 0; s0 < cnt; s0 += 4) {
#pragma unroll
        for (int s = s0; s < s0 + 4; ++s) v = __builtin_fma(-cb[s], Qm[s * WS + lane], v);
      }
    }
  };
  for (unsigned long long rem = W; rem != 0; rem &= rem - 1ull) {
    const int r = __builtin_ctzll(rem);
    // row r of D: L d^T = a_r^T, component j at lane j (0 on the padding and the upper lanes)
    double v;
    if constexpr (BX) {
      // a row >= mg is variable r - mg's unit row (r is wave-uniform: G is read below mg only)
      if (r < mg) v = var ? Aq[r * n + lane] : 0.0;
      else v = lane == r - mg ? 1.0 : 0.0;
    } else {
      v = FM == 2 ? (low ? Hg[fy.D + r * WN + lane] : 0.0) : var ? Aq[r * n + lane] : 0.0;
    }
    if constexpr (FM != 2) {
#pragma unroll
    for (int k = 0; k < WN; ++k) {
      const double dk = readlane_d(v * invLd, k);
      const double lk = (low && lane > k) ? Lm[i * WS + k] : 0.0;
      v = lane == k ? dk : __builtin_fma(-lk, dk, v);
    }
    }
    const double dd = wave_sum(low ? v * v : 0.0);
    double cl = 0.0;  // R[lane][cnt]
    project(v, cl);
    project(v, cl);
    const double nd2 = wave_sum(low ? v * v : 0.0);
    // (every lane holds the same sums; the readfirstlane tells the compiler so)
    if (__builtin_amdgcn_readfirstlane((int)(cnt < WN && nd2 > kDepTol * dd))) {
      const double rn = rsq(nd2);
      wave_lds_sync();
      if (low) Qm[cnt * WS + lane] = v * rn;
      if (lane < cnt) Lm[lane * WS + cnt] = cl;  // R above L's diagonal
      if (lane == 0) {
        ir[cnt] = rn;
        posb[r] = (double)cnt;
      }
      ++cnt;
    }
  }
  wave_lds_sync();

  if constexpr (MU) {
    // ---- T directions on the one copy of L and orthogonalisation: positions,
    // 1 / R_tt, Q and R stay in LDS, the vectors region is used again per
    // direction.  Per direction: the u loop of the factored load on the stored
    // L, and the statements below from the two projection passes to the stores.
    const Multi mu = tail_multi(glamg...);
    const double *__restrict__ gq = gxg + g * mu.stride * n + (var ? lane : 0);
    [[maybe_unused]] const double *__restrict__ glq = nullptr;
    if constexpr (DU) glq = tail_glam(glamg...) + g * mu.stride * m + (lane < m ? lane : 0);  // (the form has m > 0)
    const int p = (int)posb[lane];  // the position of row `lane`, -1: not in W or skipped
    const double invRd = lane < cnt ? ir[lane] : 0.0;
    for (int t = 0; t < mu.T; ++t) {
      const double gl = gq[(long long)t * n];
      double ut = var ? gl : 0.0;
      [[maybe_unused]] double glt = 0.0;  // glam of row `lane`, 0 outside W (whatever it holds there)
      if constexpr (DU) {
        const double v = glq[(long long)t * m];
        glt = ((W >> lane) & 1ull) ? v : 0.0;
      }
      for (int k = 0; k < n; ++k) {
        const double uk = readlane_d(ut, k) * readlane_d(invLd, k);
        const double lik = (low && lane > k) ? Lm[i * WS + k] : 0.0;
        if (lane == k) ut = uk;
        else if (low && lane > k) ut = __builtin_fma(-lik, uk, ut);
      }
      double z = low ? ut : 0.0, cu = 0.0;
      project(z, cu);
      project(z, cu);
      z = -z;
      [[maybe_unused]] double wv = 0.0;
      if constexpr (DU) {
        wave_lds_sync();
        if (low) vb[lane] = 0.0;
        wave_lds_sync();
        if (p >= 0) vb[p] = glt;
        wave_lds_sync();
        wv = lane < cnt ? vb[lane] : 0.0;
        const double iw = lane < cnt ? ir[lane] : 0.0;
        for (int s = 0; s < cnt; ++s) {
          const double wt = readlane_d(wv * iw, s);
          if (lane == s) wv = wt;
          else if (lane > s && lane < cnt) wv = __builtin_fma(-Lm[s * WS + lane], wt, wv);
        }
        wave_lds_sync();
        if (low) cb[lane] = wv;
        wave_lds_sync();
        if (low) {
          for (int s0 = 0; s0 < cnt; s0 += 4) {
#pragma unroll
            for (int s = s0; s < s0 + 4; ++s) z = __builtin_fma(-cb[s], Qm[s * WS + lane], z);
          }
        }
      }
      double y = -cu;
      if constexpr (DU) y += wv;
      for (int s = cnt - 1; s >= 0; --s) {
        const double yt = readlane_d(y * invRd, s);
        if (lane == s) y = yt;
        else if (lane < s) y = __builtin_fma(-Lm[lane * WS + s], yt, y);
      }
      double dx = z;
#pragma unroll
      for (int j = WN - 1; j >= 0; --j) {
        const double dj = readlane_d(dx * invLd, j);
        const double lj = lane < j ? Lm[j * WS + i] : 0.0;
        dx = lane == j ? dj : __builtin_fma(-lj, dj, dx);
      }
      if (!ok || !var) dx = 0.0;
      wave_lds_sync();
      if (low) cb[lane] = lane < cnt ? y : 0.0;
      wave_lds_sync();
      const double dl = p >= 0 ? cb[p] : 0.0;
      const long long qt = g * (long long)mu.T + t;
      if (gbg && lane < m) gbg[qt * m + lane] = p >= 0 ? -dl : 0.0;
      if (gfg && var) gfg[qt * n + lane] = dx;
      wave_lds_sync();  // (the next direction's passes write the vectors again)
    }
    return;
  }

  // ---- z = -(u - Q Q^T u), R dlam = -Q^T u, L^T dx = z
  // (two passes, as in the dense kernel)
  double z = low ? ub[lane] : 0.0, cu = 0.0;
  project(z, cu);
  project(z, cu);
  z = -z;
  [[maybe_unused]] double wv = 0.0;  // DU: w of position `lane` (0 past cnt)
  if constexpr (DU) {
    // g: glam of the kept rows at their positions (a skipped row has none)
    wave_lds_sync();
    if (low) vb[lane] = 0.0;
    wave_lds_sync();
    const int p = (int)posb[lane];
    if (p >= 0) vb[p] = glv;
    wave_lds_sync();
    wv = lane < cnt ? vb[lane] : 0.0;
    // R^T w = g: step t finishes w_t and the positions behind it subtract R[t][lane] w_t
    const double iw = lane < cnt ? ir[lane] : 0.0;
    for (int t = 0; t < cnt; ++t) {
      const double wt = readlane_d(wv * iw, t);
      if (lane == t) wv = wt;
      else if (lane > t && lane < cnt) wv = __builtin_fma(-Lm[t * WS + lane], wt, wv);
    }
    // z -= Q w, the last loop of a projection pass on w (the q_s past cnt are zero)
    wave_lds_sync();
    if (low) cb[lane] = wv;
    wave_lds_sync();
    if (low) {
      for (int s0 = 0; s0 < cnt; s0 += 4) {
#pragma unroll
        for (int s = s0; s < s0 + 4; ++s) z = __builtin_fma(-cb[s], Qm[s * WS + lane], z);
      }
    }
  }
  double y = -cu;  // the right-hand side, then dlam of position `lane`
  if constexpr (DU) y += wv;
  const double invRd = lane < cnt ? ir[lane] : 0.0;
  for (int t = cnt - 1; t >= 0; --t) {
    const double yt = readlane_d(y * invRd, t);
    if (lane == t) y = yt;
    else if (lane < t) y = __builtin_fma(-Lm[lane * WS + t], yt, y);
  }
  double dx = z;
#pragma unroll
  for (int j = WN - 1; j >= 0; --j) {
    const double dj = readlane_d(dx * invLd, j);
    const double lj = lane < j ? Lm[j * WS + i] : 0.0;
    dx = lane == j ? dj : __builtin_fma(-lj, dj, dx);
  }
  if (!ok || !var) dx = 0.0;

  // ------------------------------------------------------------------ store
  double *X = lds + W_X, *DX = lds + W_DX, *DL = lds + W_DL, *LM = lds + W_LM;
  wave_lds_sync();
  if (low) {
    cb[lane] = lane < cnt ? y : 0.0;
    X[lane] = (ok && var) ? xg[g * n + lane] : 0.0;
    DX[lane] = dx;
  }
  wave_lds_sync();
  {
    // row `lane`: dlam through its position, lam where its bit is set
    const int p = (int)posb[lane];
    const double dl = p >= 0 ? cb[p] : 0.0;
    const bool inW = (W >> lane) & 1ull;
    DL[lane] = dl;
    LM[lane] = inW ? lamg[g * m + lane] : 0.0;
    if constexpr (BX) {
      const Box bx = tail_box(glamg...);
      const double v = p >= 0 ? -dl : 0.0;
      if (lane < m) {
        const bool lo = bx.lower ? (bx.lower[g * words + (lane >> 5)] >> (lane & 31)) & 1u : false;
        if (lane < mg) {
          store_routed(bx.gbl, bx.gbu, g * mg + lane, lo, v);
          if (bx.gbw) bx.gbw[g * mg + lane] = v;
        } else {
          store_routed(bx.glb, bx.gub, g * n + (lane - mg), lo, v);
        }
      }
    } else {
      if (gbg && lane < m) gbg[g * m + lane] = p >= 0 ? -dl : 0.0;
    }
  }
  if (gfg && var) gfg[g * n + lane] = dx;
  wave_lds_sync();
  if (gHg) {
    double *o = gHg + g * (long long)n * n;
    for (int e = lane; e < n * n; e += 64) {
      const int row = e / n, col = e - row * n;
      o[e] = 0.5 * sym2(DX[row], X[col], X[row], DX[col]);
    }
  }
  if (gAg && ma > 0) {
    double *o = gAg + g * (long long)ma * n;
    for (int e = lane; e < ma * n; e += 64) {
      const int row = e / n, col = e - row * n;
      o[e] = sym2(DL[row], X[col], LM[row], DX[col]);
    }
  }
}

}  // namespace bwd
}  // namespace qpb

extern "C" hipError_t qpb_launch_kkt_bwd(const qpb_desc *d, const double *H, const double *A, const double *x,
                                         const double *lam, const uint32_t *active, const int32_t *status,
                                         const double *gx, double *gH, double *gf, double *gA, double *gb,
                                         hipStream_t stream) {
  if (d->n > 16 || d->m > 32) {  // one workgroup of one wave per QP
    hipLaunchKernelGGL(qpb::bwd::kkt_bwd_wave_kernel<>, dim3((unsigned)d->batch), dim3(64), 0, stream, H, A, x, lam,
                       active, status, gx, gH, gf, gA, gb, d->n, d->m, (long long)d->batch);
    return hipGetLastError();
  }
  const long long blocks = (d->batch + qpb::bwd::QPB - 1) / qpb::bwd::QPB;
  qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto) {  // (no FULL form)
    hipLaunchKernelGGL((qpb::bwd::kkt_bwd_dense_kernel<MR(), N16()>), dim3((unsigned)blocks), dim3(64), 0, stream, H,
                       A, x, lam, active, status, gx, gH, gf, gA, gb, d->n, d->m, (long long)d->batch);
  });
  return hipGetLastError();
}

// pass 1 of qpb_solve_shared_backward: the SH forms, a QP stride of 0 (one copy
// for the batch) or the batched one for each of H and A; gH / gA are NULL where
// pass 2 (qpb_kkt_bwd_sum.hip) sums the gradient
extern "C" hipError_t qpb_launch_kkt_bwd_shared(const qpb_desc *d, long long strideH, long long strideA,
                                                const double *H, const double *A, const double *x, const double *lam,
                                                const uint32_t *active, const int32_t *status, const double *gx,
                                                double *gH, double *gf, double *gA, double *gb, hipStream_t stream) {
  const int shared = (strideH == 0 ? QPB_SHARED_H : 0) | (strideA == 0 ? QPB_SHARED_A : 0);
  const int mm = d->m | (shared << qpb::bwd::kShShift);
  if (d->n > 16 || d->m > 32) {
    hipLaunchKernelGGL(qpb::bwd::kkt_bwd_wave_kernel<true>, dim3((unsigned)d->batch), dim3(64), 0, stream, H, A, x,
                       lam, active, status, gx, gH, gf, gA, gb, d->n, mm, (long long)d->batch);
    return hipGetLastError();
  }
  const long long blocks = (d->batch + qpb::bwd::QPB - 1) / qpb::bwd::QPB;
  qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto) {
    hipLaunchKernelGGL((qpb::bwd::kkt_bwd_dense_kernel<MR(), N16(), true>), dim3((unsigned)blocks), dim3(64), 0,
                       stream, H, A, x, lam, active, status, gx, gH, gf, gA, gb, d->n, mm, (long long)d->batch);
  });
  return hipGetLastError();
}

// pass 1 of qpb_solve_backward_dual (m > 0 and glam given): the DU forms, plain
// where both strides are the batched ones and SH otherwise
extern "C" hipError_t qpb_launch_kkt_bwd_dual(const qpb_desc *d, long long strideH, long long strideA,
                                              const double *H, const double *A, const double *x, const double *lam,
                                              const uint32_t *active, const int32_t *status, const double *gx,
                                              const double *glam, double *gH, double *gf, double *gA, double *gb,
                                              hipStream_t stream) {
  const int shared = (strideH == 0 ? QPB_SHARED_H : 0) | (strideA == 0 ? QPB_SHARED_A : 0);
  const int mm = d->m | (shared << qpb::bwd::kShShift);
  const long long blocks = (d->batch + qpb::bwd::QPB - 1) / qpb::bwd::QPB;
  const bool wave = d->n > 16 || d->m > 32;
  if (wave && shared) {
    hipLaunchKernelGGL(qpb::bwd::kkt_bwd_wave_kernel<true>, dim3((unsigned)d->batch), dim3(64), 0, stream, H, A, x,
                       lam, active, status, gx, gH, gf, gA, gb, d->n, mm, (long long)d->batch, glam);
  } else if (wave) {
    hipLaunchKernelGGL(qpb::bwd::kkt_bwd_wave_kernel<>, dim3((unsigned)d->batch), dim3(64), 0, stream, H, A, x, lam,
                       active, status, gx, gH, gf, gA, gb, d->n, d->m, (long long)d->batch, glam);
  } else if (shared) {
    qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto) {
      hipLaunchKernelGGL((qpb::bwd::kkt_bwd_dense_kernel<MR(), N16(), true>), dim3((unsigned)blocks), dim3(64), 0,
                         stream, H, A, x, lam, active, status, gx, gH, gf, gA, gb, d->n, mm, (long long)d->batch,
                         glam);
    });
  } else {
    qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto) {
      hipLaunchKernelGGL((qpb::bwd::kkt_bwd_dense_kernel<MR(), N16()>), dim3((unsigned)blocks), dim3(64), 0, stream,
                         H, A, x, lam, active, status, gx, gH, gf, gA, gb, d->n, d->m, (long long)d->batch, glam);
    });
  }
  return hipGetLastError();
}

// pass 1 of qpb_solve_range_box_backward: the BX forms, of the form the call on
// A' = [G; I] takes at the same arguments -- plain where both strides are the
// batched ones and SH otherwise, DU where glam is given
extern "C" hipError_t qpb_launch_kkt_bwd_range_box(const qpb_desc *d, int mg, long long strideH, long long strideG,
                                                   const double *H, const double *G, const double *x,
                                                   const double *lam, const uint32_t *active, const uint32_t *lower,
                                                   const int32_t *status, const double *gx, const double *glam,
                                                   double *gH, double *gf, double *gG, double *gbl, double *gbu,
                                                   double *glb, double *gub, double *gbw, hipStream_t stream) {
  const int shared = (strideH == 0 ? QPB_SHARED_H : 0) | ((strideG == 0 && mg > 0) ? QPB_SHARED_A : 0);
  const int mm = d->m | (shared << qpb::bwd::kShShift);
  const long long blocks = (d->batch + qpb::bwd::QPB - 1) / qpb::bwd::QPB;
  const bool wave = d->n > 16 || d->m > 32;
  const qpb::bwd::Box bx{mg, lower, gbl, gbu, glb, gub, gbw};
  double *no_gb = nullptr;
  auto go = [&](auto... tail) {
    if (wave && shared) {
      hipLaunchKernelGGL(qpb::bwd::kkt_bwd_wave_kernel<true>, dim3((unsigned)d->batch), dim3(64), 0, stream, H, G, x,
                         lam, active, status, gx, gH, gf, gG, no_gb, d->n, mm, (long long)d->batch, tail...);
    } else if (wave) {
      hipLaunchKernelGGL(qpb::bwd::kkt_bwd_wave_kernel<>, dim3((unsigned)d->batch), dim3(64), 0, stream, H, G, x, lam,
                         active, status, gx, gH, gf, gG, no_gb, d->n, d->m, (long long)d->batch, tail...);
    } else if (shared) {
      qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto) {
        hipLaunchKernelGGL((qpb::bwd::kkt_bwd_dense_kernel<MR(), N16(), true>), dim3((unsigned)blocks), dim3(64), 0,
                           stream, H, G, x, lam, active, status, gx, gH, gf, gG, no_gb, d->n, mm, (long long)d->batch,
                           tail...);
      });
    } else {
      qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto) {
        hipLaunchKernelGGL((qpb::bwd::kkt_bwd_dense_kernel<MR(), N16()>), dim3((unsigned)blocks), dim3(64), 0, stream,
                           H, G, x, lam, active, status, gx, gH, gf, gG, no_gb, d->n, d->m, (long long)d->batch,
                           tail...);
      });
    }
  };
  if (glam) go(glam, bx);
  else go(bx);
  return hipGetLastError();
}

// qpb_factor_shared_backward: one launch of one workgroup of the class's own
// kernel in its factor form, on the one H and A
extern "C" hipError_t qpb_launch_kkt_bwd_factor(int n, int m, const double *H, const double *A, double *bfac,
                                                int32_t *fstatus, hipStream_t stream) {
  double *const found = reinterpret_cast<double *>(fstatus);  // the form's one int32 output
  const double *no_d = nullptr;
  const uint32_t *no_u = nullptr;
  const int32_t *no_i = nullptr;
  double *no_o = nullptr;
  if (n > 16 || m > 32) {
    hipLaunchKernelGGL((qpb::bwd::kkt_bwd_wave_kernel<false, qpb::bwd::Form<1>>), dim3(1), dim3(64), 0, stream, H, A, no_d, no_d, no_u,
                       no_i, no_d, bfac, no_o, no_o, found, n, m, 1LL);
    return hipGetLastError();
  }
  qpb::row16::dispatch_form(n, m, [&](auto MR, auto N16, auto) {
    hipLaunchKernelGGL((qpb::bwd::kkt_bwd_dense_kernel<MR(), N16(), false, qpb::bwd::Form<1>>), dim3(1), dim3(64), 0, stream, H, A,
                       no_d, no_d, no_u, no_i, no_d, bfac, no_o, no_o, found, n, m, 1LL);
  });
  return hipGetLastError();
}

// pass 1 of qpb_solve_factored_backward: the factored forms on such a buffer
// (gH and gA are pass 2's)
extern "C" hipError_t qpb_launch_kkt_bwd_factored(const qpb_desc *d, const double *bfac, const double *x,
                                                  const double *lam, const uint32_t *active, const int32_t *status,
                                                  const double *gx, double *gf, double *gb, hipStream_t stream) {
  const double *no_a = nullptr;
  double *no_o = nullptr;
  if (d->n > 16 || d->m > 32) {
    hipLaunchKernelGGL((qpb::bwd::kkt_bwd_wave_kernel<false, qpb::bwd::Form<2>>), dim3((unsigned)d->batch), dim3(64), 0, stream, bfac,
                       no_a, x, lam, active, status, gx, no_o, gf, no_o, gb, d->n, d->m, (long long)d->batch);
    return hipGetLastError();
  }
  const long long blocks = (d->batch + qpb::bwd::QPB - 1) / qpb::bwd::QPB;
  qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto) {
    hipLaunchKernelGGL((qpb::bwd::kkt_bwd_dense_kernel<MR(), N16(), false, qpb::bwd::Form<2>>), dim3((unsigned)blocks), dim3(64), 0,
                       stream, bfac, no_a, x, lam, active, status, gx, no_o, gf, no_o, gb, d->n, d->m,
                       (long long)d->batch);
  });
  return hipGetLastError();
}

// pass 1 of qpb_solve_factored_backward_dual (m > 0 and glam given): the DU
// forms of the factored forms
extern "C" hipError_t qpb_launch_kkt_bwd_factored_dual(const qpb_desc *d, const double *bfac, const double *x,
                                                       const double *lam, const uint32_t *active,
                                                       const int32_t *status, const double *gx, const double *glam,
                                                       double *gf, double *gb, hipStream_t stream) {
  const double *no_a = nullptr;
  double *no_o = nullptr;
  if (d->n > 16 || d->m > 32) {
    hipLaunchKernelGGL((qpb::bwd::kkt_bwd_wave_kernel<false, qpb::bwd::Form<2>>), dim3((unsigned)d->batch), dim3(64), 0, stream, bfac,
                       no_a, x, lam, active, status, gx, no_o, gf, no_o, gb, d->n, d->m, (long long)d->batch, glam);
    return hipGetLastError();
  }
  const long long blocks = (d->batch + qpb::bwd::QPB - 1) / qpb::bwd::QPB;
  qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto) {
    hipLaunchKernelGGL((qpb::bwd::kkt_bwd_dense_kernel<MR(), N16(), false, qpb::bwd::Form<2>>), dim3((unsigned)blocks), dim3(64), 0,
                       stream, bfac, no_a, x, lam, active, status, gx, no_o, gf, no_o, gb, d->n, d->m,
                       (long long)d->batch, glam);
  });
  return hipGetLastError();
}

// qpb_solve_factored_backward_multi: the MU forms of the factored forms, with
// glam (d->m > 0: the DU MU forms) or without; T directions per QP, the
// right-hand sides' QP stride in directions rstride (T, or 0: one set for the batch)
extern "C" hipError_t qpb_launch_kkt_bwd_factored_multi(const qpb_desc *d, const double *bfac, const uint32_t *active,
                                                        const int32_t *status, int T, long long rstride,
                                                        const double *gx, const double *glam, double *gf, double *gb,
                                                        hipStream_t stream) {
  using qpb::bwd::Form;
  const qpb::bwd::Multi mu{T, rstride};
  const double *no_a = nullptr;
  double *no_o = nullptr;
  if (d->n > 16 || d->m > 32) {
    auto go = [&](auto... tail) {
      hipLaunchKernelGGL((qpb::bwd::kkt_bwd_wave_kernel<false, Form<2>>), dim3((unsigned)d->batch), dim3(64), 0, stream,
                         bfac, no_a, no_a, no_a, active, status, gx, no_o, gf, no_o, gb, d->n, d->m,
                         (long long)d->batch, tail...);
    };
    if (glam) go(glam, mu);
    else go(mu);
    return hipGetLastError();
  }
  const long long blocks = (d->batch + qpb::bwd::QPB - 1) / qpb::bwd::QPB;
  qpb::row16::dispatch_form(d->n, d->m, [&](auto MR, auto N16, auto) {
    auto go = [&](auto... tail) {
      hipLaunchKernelGGL((qpb::bwd::kkt_bwd_dense_kernel<MR(), N16(), false, Form<2>>), dim3((unsigned)blocks),
                         dim3(64), 0, stream, bfac, no_a, no_a, no_a, active, status, gx, no_o, gf, no_o, gb, d->n,
                         d->m, (long long)d->batch, tail...);
    };
    if (glam) go(glam, mu);
    else go(mu);
  });
  return hipGetLastError();
}
