// qpb_kkt_bwd_box.hip -- the backward pass of a box solve (qpb_solve_box_backward)
// for gfx950.
//
// For lb <= x <= ub the active rows are unit vectors, and the KKT system at a
// fixed active set collapses.  Variable j is FIXED when its upper-bound bit
// (j) or its lower-bound bit (n + j) is set in the active mask W; F are the
// free variables.  With the cotangent g = dl/dx,
//
//     dx_fixed = 0                 H_FF dx_F = -g_F
//     r = g + H dx                 (zero on F by construction)
//     dl/df = dx                   dl/dH = 1/2 (dx x^T + x dx^T)
//     dl/dub_j = r_j  if the upper bound of j is active, else 0
//     dl/dlb_j = r_j  if the lower bound of j is active and the upper is not, else 0
//
// One Cholesky of a principal submatrix of H, two triangular solves and one
// matrix-vector product: no A, no lam, no orthogonalisation, no R.
//
// The free block is factored WITHOUT a gather: a fixed (or padded) variable's
// row of H is replaced by the unit row e_j, its column is zeroed in every
// other row, and its cotangent becomes 0.  The Cholesky factor of that matrix
// is the factor of H_FF with identity rows and columns threaded through it,
// and the two solves leave exact zeros on the fixed variables.  This is the
// identity padding of n < 16 (row16::h_padded), driven by the mask.
//
// n <= 16 (kkt_bwd_box_dense_kernel): kkt_bwd_dense_kernel's mapping, one QP
// per 16-lane DPP row, four per wavefront, in the LDS slot and with the
// shared steps of qpb_row16.h.  Lane l holds row l of H twice: untouched (for
// r) and masked (it becomes row l of L in the right-looking DPP sweep).
// Every loop bound is a compile-time constant.
// 16 < n <= 32 (kkt_bwd_box_wave_kernel): one QP per wavefront, L in a 32 x 33
// LDS block in kkt_bwd_wave_kernel's manner, the untouched H in a second one.
#include "qpb_launch.h"  // with qpb.h
#include "qpb_row16.h"

namespace qpb {
namespace bwdbox {
using namespace row16;

// the vectors of the outer product, over the dead L
constexpr int OFF_X = 0, OFF_DX = 16;
static_assert(OFF_DX + 16 <= L_SIZE, "the output vectors fit the dead L");

// p + q rounded once each and added: the value is symmetric under swapping the
// two products, so gH == gH^T bit for bit (a contracted fma(a, b, c d) is not)
__device__ __forceinline__ double sym2(double a, double b, double c, double d) {
#pragma clang fp contract(off)
  const double p = a * b;
  const double q = c * d;
  return p + q;
}

// N16: n == 16 (coalesced loads and stores through this QP's LDS slot);
// otherwise the rows are padded with the identity.
// SH (pass 1 of qpb_solve_box_shared_backward, both kernels): the QP stride of
// H, in doubles, is the one trailing argument that only this form has, the
// run-time strideH -- 0 for one H that the whole batch shares, or n n.  The
// masked factorisation differs per QP and stays per QP; only the address of H
// changes, so gf, glb and gub are the other form's bit for bit.  The form's
// gHg is per QP like the other's (pass 1 passes NULL: the sum is pass 2's).
// Without SH the pack is empty: the signatures and code objects stay.
// DU (qpb_solve_box_backward_dual, both kernels, plain and SH): the cotangent
// glam on the multipliers, B x 2n in qpb_solve_box's lam layout (the upper
// bounds' entries, then the lower bounds'), is the pack's last argument, a
// const double *, which only this form has.  On unit rows it prescribes dx on
// the fixed variables: d_j = -glam[j] where the upper bit of j is set,
// +glam[n + j] where only the lower bit is, 0 on a free variable, and
//
//     dx_S = d_S                   H_FF dx_F = -g_F - H_FS d_S
//
// with r, and every output's formula, as above.  The masked Cholesky is the
// same; the new work is d, one product of the untouched rows of H with it, and
// d on the fixed lanes where the other forms store zeros.
// MU (qpb_solve_box_backward_multi, both kernels, on the SH forms' run-time
// stride of H, with and without glam): T right-hand sides per QP.  The pack's
// last argument, a Multi, which only this form has, carries T and the QP stride
// of the right-hand sides in directions (T, or 0 for one set that the whole
// batch reads).  Direction t of QP k reads gx + (k stride + t) n and glam +
// (k stride + t) 2n and writes gf, glb, gub + (k T + t) n.  The load of H, the
// mask and the masked Cholesky run once; the untouched rows, L, 1 / L_kk and
// the mask stay where they are, and a loop over t repeats the rest of the
// single-direction form operation for operation, so every direction's bits
// are that form's.  x and gH are not arguments of the call: NULL, never read.
struct Multi {
  int T;
  long long stride;
};
template <bool SH, class... EX>
inline constexpr bool extra_pack_ok =
    SH ? (std::is_same_v<void(EX...), void(long long)> || std::is_same_v<void(EX...), void(long long, const double *)> ||
          std::is_same_v<void(EX...), void(long long, Multi)> ||
          std::is_same_v<void(EX...), void(long long, const double *, Multi)>)
       : (std::is_same_v<void(EX...), void()> || std::is_same_v<void(EX...), void(const double *)>);
template <class... EX>
inline constexpr bool pack_is_multi = (std::is_same_v<EX, Multi> || ...);
template <class... T>
__device__ __forceinline__ long long pack_stride(long long s, T...) {
  return s;
}
__device__ __forceinline__ const double *pack_glam(const double *p) { return p; }
__device__ __forceinline__ const double *pack_glam(long long, const double *p) { return p; }
__device__ __forceinline__ const double *pack_glam(long long, const double *p, Multi) { return p; }
__device__ __forceinline__ Multi pack_multi(long long, Multi mu) { return mu; }
__device__ __forceinline__ Multi pack_multi(long long, const double *, Multi mu) { return mu; }

template <bool N16, bool SH = false, class... EX>
__global__ __launch_bounds__(64, 3) void kkt_bwd_box_dense_kernel(
    const double *__restrict__ Hg, const double *__restrict__ xg, const uint32_t *__restrict__ actg,
    const int32_t *__restrict__ statg, const double *__restrict__ gxg, double *__restrict__ gHg,
    double *__restrict__ gfg, double *__restrict__ glbg, double *__restrict__ gubg, int n, long long batch,
    EX... extra) {
  static_assert(extra_pack_ok<SH, EX...>,
                "the shared form alone takes the stride, the dual form glam behind it, the multi form a Multi last");
  constexpr bool MU = pack_is_multi<EX...>;
  constexpr bool DU = sizeof...(EX) - (MU ? 1 : 0) == (SH ? 2 : 1);
  __shared__ double lds[QPB * SLOT];
  const int l = threadIdx.x & (NL - 1);
  const int slot = threadIdx.x >> 4;
  const auto [live, g] = ragged_qp(blockIdx.x, slot, batch);
  if constexpr (N16) n = NL;
  double *base = slot_base(lds, slot);
  double *Lp = base + OFF_L;
  double *xcap = base + OFF_R;  // the solves' captured components (16)

  // ------------------------------------------------------------------ load
  const bool var = N16 || l < n;
  const int lc = var ? l : n - 1;
  const double *Hq;
  if constexpr (SH)
    Hq = Hg + g * pack_stride(extra...);
  else
    Hq = Hg + g * (long long)n * n;
  const bool ok = statg ? statg[g] == QPB_OK : true;
  // a QP that is not QPB_OK has no fixed variable and stores zeros
  const uint32_t W = ok ? actg[g] : 0u;
  const uint32_t nmask = (1u << n) - 1u;  // n <= 16
  const uint32_t fixed = (W | (W >> n)) & nmask;
  double gv = 0.0, xv = 0.0;  // (MU: per direction, below; no x)
  if constexpr (!MU) {
    gv = gxg[g * n + lc];
    xv = xg[g * n + lc];
  }
  [[maybe_unused]] double dv = 0.0;  // DU: the prescribed dx of a fixed variable, 0 on a free or padded one
  if constexpr (DU && !MU) {
    // both entries are loaded and one is selected: whatever glam holds at a
    // clear bit, NaN included, goes nowhere
    const double *__restrict__ glq = pack_glam(extra...) + g * (long long)(2 * n);
    const double gu = glq[lc], gw = glq[n + lc];
    const bool bu = var && ((W >> l) & 1u), bl = var && ((W >> (l + n)) & 1u);
    dv = bu ? -gu : (bl ? gw : 0.0);
  }
  double Hr[NL];  // row l of H, untouched
  if constexpr (N16) {
    // coalesced 16-byte loads, two whole rows of each of the wave's 4 QPs per
    // instruction; the rows reach their owner lanes through a transpose in
    // this QP's LDS slot (qpb_kkt_bwd.hip)
    const int hr = l >> 3, hc = 2 * (l & 7);
    double2 hv[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) hv[t] = *reinterpret_cast<const double2 *>(&Hq[(2 * t + hr) * NL + hc]);
    wave_lds_sync();
#pragma unroll
    for (int t = 0; t < 8; ++t) *reinterpret_cast<double2 *>(&base[(2 * t + hr) * RS + hc]) = hv[t];
    wave_lds_sync();
    lds_row16(&base[l * RS], Hr);
    wave_lds_sync();
  } else {
#pragma unroll
    for (int j = 0; j < NL; ++j) Hr[j] = h_padded(Hq, l, lc, n, j);
  }
  // the masked matrix: e_l on a fixed or padded lane, zero in fixed columns
  // (the padded columns are zero already)
  const bool fix = !var || ((fixed >> l) & 1u);
  double Lr[NL];  // becomes row l of L
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const double unit = l == j ? 1.0 : 0.0;
    Lr[j] = fix ? unit : (((fixed >> j) & 1u) ? 0.0 : Hr[j]);
  }

  // ---- H~ = L L^T: kkt_bwd_dense_kernel's right-looking sweep without its E
  // rows.  Step k: the pivot row is read straight from lane k by the DPP-fused
  // FMAs; the sched_barrier and the rsq chain keep every write of Lr[j]
  // (previous step) well over two instructions before these reads.
  double invLd = 0.0;
  unroll<NL>([&](auto K) {
    constexpr int k = K;
    __builtin_amdgcn_sched_barrier(0);
    const double akk = bc<k>(Lr[k]);
    const double ik = rsq1(akk);
    const double ik2 = ik * ik;
    const double nc = -(Lr[k] * ik2);
    invLd = l == k ? ik : invLd;
    pin(invLd);
    unroll<NL - 1 - k>([&](auto J) {
      constexpr int j = k + 1 + J;
      fmac_bc<k>(Lr[j], Lr[j], nc);
    });
    Lr[k] *= ik;
    pin(Lr[k]);
  });
  __builtin_amdgcn_sched_barrier(0);
  store_l(Lp, l, Lr);  // for the second solve

  if constexpr (MU) {
    // ---- T directions on the one factorisation: the statements below, from
    // the loads of gx and glam to the three stores, once per direction
    const Multi mu = pack_multi(extra...);
    const double *__restrict__ gq = gxg + g * mu.stride * n + lc;
    [[maybe_unused]] const double *__restrict__ glq = nullptr;
    if constexpr (DU) glq = pack_glam(extra...) + g * mu.stride * (2 * n) + lc;
    const long long o0 = g * (long long)mu.T * n + l;
    const bool bu = var && ((W >> l) & 1u), bl = var && ((W >> (l + n)) & 1u);
    const bool up = (W >> l) & 1u, lo = (W >> (l + n)) & 1u;
    for (int t = 0; t < mu.T; ++t) {
      const double gt = gq[(long long)t * n];
      [[maybe_unused]] double dt = 0.0;
      if constexpr (DU) {
        const double gu = glq[(long long)t * (2 * n)], gw = glq[(long long)t * (2 * n) + n];
        dt = bu ? -gu : (bl ? gw : 0.0);
      }
      double rhs = gt;
      if constexpr (DU) {
        pin(dt);
        dpp_ready(dt);
        unroll<NL>([&](auto K) { fmac_bc<K>(rhs, dt, Hr[K]); });
      }
      double dx = solve_x(fix ? 0.0 : rhs, invLd, Lr, Lp, l, xcap);
      if (fix || !ok) dx = 0.0;
      if constexpr (DU) dx = fix ? dt : dx;
      double r = gt;
      pin(dx);
      dpp_ready(dx);
      unroll<NL>([&](auto K) { fmac_bc<K>(r, dx, Hr[K]); });
      if (live && var) {
        const long long o = o0 + (long long)t * n;
        if (gfg) gfg[o] = dx;
        if (gubg) gubg[o] = up ? r : 0.0;
        if (glbg) glbg[o] = (lo && !up) ? r : 0.0;
      }
      wave_lds_sync();  // (the next direction's solves write the captured components again)
    }
    return;
  }

  // ---- dx = -H~^{-1} g~: exact zeros on the fixed lanes
  double rhs = gv;
  if constexpr (DU) {
    // g_F + H_FS d_S: d is zero off S, so the whole untouched row serves; d_k
    // is read from lane k by the FMA, as dx is for r below
    pin(dv);
    dpp_ready(dv);
    unroll<NL>([&](auto K) { fmac_bc<K>(rhs, dv, Hr[K]); });
  }
  double dx = solve_x(fix ? 0.0 : rhs, invLd, Lr, Lp, l, xcap);
  if (fix || !ok) dx = 0.0;
  // (DU: the fixed lanes' identity rows would carry d through the two solves
  // times 1 / sqrt(1) twice; the select keeps dx_S = d_S to the bit whatever
  // that rounds to.  d is 0 on a QP that is not QPB_OK: it has no fixed variable)
  if constexpr (DU) dx = fix ? dv : dx;
  // ---- r = g + H dx from the untouched row, dx_k read from lane k by the FMA
  double r = gv;
  pin(dx);
  dpp_ready(dx);
  unroll<NL>([&](auto K) { fmac_bc<K>(r, dx, Hr[K]); });

  // ------------------------------------------------------------------ store
  const bool up = (W >> l) & 1u, lo = (W >> (l + n)) & 1u;
  if (live && var) {
    if (gfg) gfg[g * n + l] = dx;
    if (gubg) gubg[g * n + l] = up ? r : 0.0;
    if (glbg) glbg[g * n + l] = (lo && !up) ? r : 0.0;
  }
  if (!gHg) return;  // wave-uniform
  // the vectors of the outer product, over the dead L
  wave_lds_sync();
  base[OFF_X + l] = (ok && var) ? xv : 0.0;
  base[OFF_DX + l] = dx;
  wave_lds_sync();
  const double *X = base + OFF_X, *DX = base + OFF_DX;
  if constexpr (N16) {
    // lane l writes columns 2 (l & 7), +1 of rows 2 t + (l >> 3): 256 contiguous bytes per QP and store
    const int hr = l >> 3, hc = 2 * (l & 7);
    const double x0 = X[hc], x1 = X[hc + 1], d0 = DX[hc], d1 = DX[hc + 1];
    if (live) {
      double *o = gHg + g * (long long)(NL * NL);
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int row = 2 * t + hr;
        const double dr = DX[row], xr = X[row];
        *reinterpret_cast<double2 *>(&o[row * NL + hc]) =
            make_double2(0.5 * sym2(dr, x0, xr, d0), 0.5 * sym2(dr, x1, xr, d1));
      }
    }
  } else {
    // element e of the row-major output at lane e mod 16
    if (live) {
      double *o = gHg + g * (long long)n * n;
      for (int e = l; e < n * n; e += NL) {
        const int row = e / n, col = e - row * n;
        o[e] = 0.5 * sym2(DX[row], X[col], X[row], DX[col]);
      }
    }
  }
}

// ---- 16 < n <= 32: one QP per wavefront ---------------------------------------
// kkt_bwd_wave_kernel's layout: L in the lower triangle of a 32 x 33 block (odd
// stride: rows and columns are both conflict-free), the untouched H in a
// second block for r.  H is padded to 32 x 32 with the identity, and the fixed
// variables are padding inside it: the same loops with the same constant
// bounds.  Lane j < 32 holds component j of the running vectors.
constexpr int WN = 32;      // variables (lanes that carry a component)
constexpr int WS = WN + 1;  // row stride
constexpr int W_L = 0, W_H = WN * WS, W_X = 2 * WN * WS, W_DX = W_X + 32, W_SIZE = W_DX + 32;
constexpr int W_COL = WN + 2;  // the pivot column of a factorisation step, zero past the matrix
static_assert((W_SIZE + W_COL) * 8 <= 20480, "8 waves per CU by LDS");

template <bool SH = false, class... EX>
__global__ __launch_bounds__(64) void kkt_bwd_box_wave_kernel(
    const double *__restrict__ Hg, const double *__restrict__ xg, const uint32_t *__restrict__ actg,
    const int32_t *__restrict__ statg, const double *__restrict__ gxg, double *__restrict__ gHg,
    double *__restrict__ gfg, double *__restrict__ glbg, double *__restrict__ gubg, int n, long long batch,
    EX... extra) {
  static_assert(extra_pack_ok<SH, EX...>,
                "the shared form alone takes the stride, the dual form glam behind it, the multi form a Multi last");
  constexpr bool MU = pack_is_multi<EX...>;
  constexpr bool DU = sizeof...(EX) - (MU ? 1 : 0) == (SH ? 2 : 1);
  __shared__ double lds[W_SIZE];
  // an object of its own: the factorisation's trailing update reads it while
  // it writes L, and the compiler can then batch the reads of an unrolled trip
  __shared__ double colk[W_COL];
  const int lane = threadIdx.x;
  const int i = lane & (WN - 1), half = lane >> 5;
  const bool low = lane < WN;      // the lanes that carry a component
  const long long g = blockIdx.x;  // one workgroup of one wave per QP: always < batch
  double *Lm = lds + W_L, *Hm = lds + W_H, *X = lds + W_X, *DX = lds + W_DX;
  const double *Hq;
  if constexpr (SH)
    Hq = Hg + g * pack_stride(extra...);
  else
    Hq = Hg + g * (long long)n * n;
  const bool ok = statg ? statg[g] == QPB_OK : true;
  // The active mask as one 64-bit word (wave-uniform): 16 < n, so 2n bits
  // take two words, and bit n + j of a lower bound crosses from word 0 into
  // word 1 at j = 32 - n.  A QP that is not QPB_OK has no fixed variable.
  unsigned long long W = 0;
  if (ok) {
    W = actg[g * 2] | ((unsigned long long)actg[g * 2 + 1] << 32);
    if (n < 32) W &= (1ull << (2 * n)) - 1ull;
  }
  const uint32_t nmask = (uint32_t)((1ull << n) - 1ull);
  const uint32_t upw = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)W & nmask));
  const uint32_t low_w = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(W >> n) & nmask));
  const uint32_t fixed = upw | low_w;
  // H untouched (zero padding) and masked: e_j on a fixed or padded variable, zero in its column
  for (int e = lane; e < WN * WN; e += 64) {
    const int row = e >> 5, col = e & (WN - 1);
    const bool in = row < n && col < n;
    const double h = Hq[in ? row * n + col : 0];
    const bool fx = !in || ((fixed >> row) & 1u) || ((fixed >> col) & 1u);
    Hm[row * WS + col] = in ? h : 0.0;
    Lm[row * WS + col] = fx ? (row == col ? 1.0 : 0.0) : h;
  }
  if (lane < W_COL) colk[lane] = 0.0;
  const bool var = lane < n;
  const bool fix = !var || ((fixed >> i) & 1u);  // (lane < n <= 32: i == lane)
  double gv = 0.0;  // (MU: per direction, below)
  if constexpr (!MU) gv = var ? gxg[g * n + lane] : 0.0;
  [[maybe_unused]] double dv = 0.0;  // DU: the prescribed dx of a fixed variable, 0 on a free or padded one
  if constexpr (DU && !MU) {
    // both entries are loaded and one is selected: whatever glam holds at a
    // clear bit, NaN included, goes nowhere
    const double *__restrict__ glq = pack_glam(extra...) + g * (long long)(2 * n);
    const int lc = var ? lane : 0;
    const double gu = glq[lc], gw = glq[n + lc];
    const bool bu = var && ((upw >> i) & 1u), bl = var && ((low_w >> i) & 1u);
    dv = bu ? -gu : (bl ? gw : 0.0);
    if (low) DX[lane] = dv;
  }
  double ui = fix ? 0.0 : gv;       // the running g~, u_k = (L^{-1} g~)_k from step k on
  double invLd = var ? 0.0 : 1.0;   // 1 / L[lane][lane] (1 on the padding)
  wave_lds_sync();
  if constexpr (MU) {
    // ---- H~ = L L^T alone, by the loop below without its u; then T directions
    // on it.  A direction takes u = L^{-1} g~ from the stored L and 1 / L_kk by
    // that loop's own operations on u (as kkt_bwd_wave_kernel does on a factor
    // buffer), and the rest is the single-direction form's, statement for
    // statement, from the loads of gx and glam to the three stores.
    for (int k = 0; k < n; ++k) {
      const double ik = rsq(Lm[k * WS + k]);
      const double lik = i >= k ? Lm[i * WS + k] * ik : 0.0;
      wave_lds_sync();
      if (half == 0) {
        colk[i] = i > k ? lik : 0.0;
        if (i >= k) Lm[i * WS + k] = lik;
      }
      if (lane == k) invLd = ik;
      wave_lds_sync();
      const double nl = i > k ? -lik : 0.0;
      double *row = Lm + i * WS + k + 1 + half;
      const double *col = colk + k + 1 + half;
      const int trips = (WN - k) / 2;
#pragma unroll 4
      for (int jj = 0; jj < trips; ++jj) row[2 * jj] = __builtin_fma(nl, col[2 * jj], row[2 * jj]);
      wave_lds_sync();
    }
    const Multi mu = pack_multi(extra...);
    const int lc = var ? lane : 0;
    const double *__restrict__ gq = gxg + g * mu.stride * n + lc;
    [[maybe_unused]] const double *__restrict__ glq = nullptr;
    if constexpr (DU) glq = pack_glam(extra...) + g * mu.stride * (2 * n) + lc;
    const bool up = (upw >> i) & 1u, lo = (low_w >> i) & 1u;  // (used on lanes < n: i == lane)
    for (int t = 0; t < mu.T; ++t) {
      const double gl = gq[(long long)t * n];
      const double gt = var ? gl : 0.0;
      [[maybe_unused]] double dt = 0.0;
      if constexpr (DU) {
        const double gu = glq[(long long)t * (2 * n)], gw = glq[(long long)t * (2 * n) + n];
        dt = (var && up) ? -gu : ((var && lo) ? gw : 0.0);
        if (low) DX[lane] = dt;
        wave_lds_sync();
      }
      double ut = fix ? 0.0 : gt;
      if constexpr (DU) {
        if (!fix) {
          double r0 = gt, r1 = 0.0;
#pragma unroll
          for (int j = 0; j < WN; j += 2) {
            r0 = __builtin_fma(Hm[lane * WS + j], DX[j], r0);
            r1 = __builtin_fma(Hm[lane * WS + j + 1], DX[j + 1], r1);
          }
          ut = r0 + r1;
        }
      }
      for (int k = 0; k < n; ++k) {
        const double uk = readlane_d(ut, k) * readlane_d(invLd, k);
        const double lik = (low && lane > k) ? Lm[i * WS + k] : 0.0;
        if (lane == k) ut = uk;
        else if (low && lane > k) ut = __builtin_fma(-lik, uk, ut);
      }
      double dx = low ? -ut : 0.0;
#pragma unroll
      for (int j = WN - 1; j >= 0; --j) {
        const double dj = readlane_d(dx * invLd, j);
        const double lj = lane < j ? Lm[j * WS + i] : 0.0;
        dx = lane == j ? dj : __builtin_fma(-lj, dj, dx);
      }
      if (!ok || fix) dx = 0.0;
      if constexpr (DU) dx = fix ? dt : dx;
      wave_lds_sync();
      if (low) DX[lane] = dx;
      wave_lds_sync();
      if (var) {
        double r0 = gt, r1 = 0.0;
#pragma unroll
        for (int j = 0; j < WN; j += 2) {
          r0 = __builtin_fma(Hm[lane * WS + j], DX[j], r0);
          r1 = __builtin_fma(Hm[lane * WS + j + 1], DX[j + 1], r1);
        }
        const double r = r0 + r1;
        const long long o = (g * (long long)mu.T + t) * n + lane;
        if (gfg) gfg[o] = dx;
        if (gubg) gubg[o] = up ? r : 0.0;
        if (glbg) glbg[o] = (lo && !up) ? r : 0.0;
      }
      wave_lds_sync();  // (the next direction writes DX again)
    }
    return;
  }
  if constexpr (DU) {
    // g~_F = g_F + H_FS d_S: d is zero off S, so the whole untouched row
    // serves, by the loop of r below
    if (!fix) {
      double r0 = gv, r1 = 0.0;
#pragma unroll
      for (int j = 0; j < WN; j += 2) {
        r0 = __builtin_fma(Hm[lane * WS + j], DX[j], r0);
        r1 = __builtin_fma(Hm[lane * WS + j + 1], DX[j + 1], r1);
      }
      ui = r0 + r1;
    }
  }

  // ---- H~ = L L^T (right-looking, in place) and u = L^{-1} g~: kkt_bwd_wave_kernel's
  // loop.  Step k updates the whole rows k+1.. of the symmetric trailing
  // block, the two halves of the wave on alternate columns (the last trip of
  // the upper half may touch the row's padding word, colk is zero there)
  for (int k = 0; k < n; ++k) {
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

  // ---- L^T dx = -u
  double dx = low ? -ui : 0.0;
#pragma unroll
  for (int j = WN - 1; j >= 0; --j) {
    const double dj = readlane_d(dx * invLd, j);
    const double lj = lane < j ? Lm[j * WS + i] : 0.0;
    dx = lane == j ? dj : __builtin_fma(-lj, dj, dx);
  }
  if (!ok || fix) dx = 0.0;
  // (DU: dx_S = d_S to the bit; d is 0 on the padding and on a QP that is not
  // QPB_OK, which has no fixed variable)
  if constexpr (DU) dx = fix ? dv : dx;
  if (low) {
    X[lane] = (ok && var) ? xg[g * n + lane] : 0.0;
    DX[lane] = dx;
  }
  wave_lds_sync();

  // ---- r = g + H dx from the untouched rows (zero past n)
  if (var) {
    double r0 = gv, r1 = 0.0;
#pragma unroll
    for (int j = 0; j < WN; j += 2) {
      r0 = __builtin_fma(Hm[lane * WS + j], DX[j], r0);
      r1 = __builtin_fma(Hm[lane * WS + j + 1], DX[j + 1], r1);
    }
    const double r = r0 + r1;
    const bool up = (upw >> lane) & 1u, lo = (low_w >> lane) & 1u;
    if (gfg) gfg[g * n + lane] = dx;
    if (gubg) gubg[g * n + lane] = up ? r : 0.0;
    if (glbg) glbg[g * n + lane] = (lo && !up) ? r : 0.0;
  }
  if (gHg) {
    double *o = gHg + g * (long long)n * n;
    for (int e = lane; e < n * n; e += 64) {
      const int row = e / n, col = e - row * n;
      o[e] = 0.5 * sym2(DX[row], X[col], X[row], DX[col]);
    }
  }
}

}  // namespace bwdbox
}  // namespace qpb

extern "C" hipError_t qpb_launch_kkt_bwd_box(const qpb_desc *d, const double *H, const double *x,
                                             const uint32_t *active, const int32_t *status, const double *gx,
                                             double *gH, double *gf, double *glb, double *gub, hipStream_t stream) {
  using namespace qpb::bwdbox;
  if (d->n > 16) {  // one workgroup of one wave per QP
    hipLaunchKernelGGL(kkt_bwd_box_wave_kernel<>, dim3((unsigned)d->batch), dim3(64), 0, stream, H, x, active, status,
                       gx, gH, gf, glb, gub, d->n, (long long)d->batch);
    return hipGetLastError();
  }
  const long long blocks = (d->batch + QPB - 1) / QPB;
  if (d->n == 16)
    hipLaunchKernelGGL(kkt_bwd_box_dense_kernel<true>, dim3((unsigned)blocks), dim3(64), 0, stream, H, x, active,
                       status, gx, gH, gf, glb, gub, d->n, (long long)d->batch);
  else
    hipLaunchKernelGGL(kkt_bwd_box_dense_kernel<false>, dim3((unsigned)blocks), dim3(64), 0, stream, H, x, active,
                       status, gx, gH, gf, glb, gub, d->n, (long long)d->batch);
  return hipGetLastError();
}

// pass 1 of qpb_solve_box_shared_backward: the SH forms, H's QP stride at run
// time (0: one copy for the batch, or n n); gH, where given, is per QP
extern "C" hipError_t qpb_launch_kkt_bwd_box_shared(const qpb_desc *d, long long strideH, const double *H,
                                                    const double *x, const uint32_t *active, const int32_t *status,
                                                    const double *gx, double *gH, double *gf, double *glb,
                                                    double *gub, hipStream_t stream) {
  using namespace qpb::bwdbox;
  if (d->n > 16) {
    hipLaunchKernelGGL((kkt_bwd_box_wave_kernel<true, long long>), dim3((unsigned)d->batch), dim3(64), 0, stream, H, x,
                       active, status, gx, gH, gf, glb, gub, d->n, (long long)d->batch, strideH);
    return hipGetLastError();
  }
  const long long blocks = (d->batch + QPB - 1) / QPB;
  if (d->n == 16)
    hipLaunchKernelGGL((kkt_bwd_box_dense_kernel<true, true, long long>), dim3((unsigned)blocks), dim3(64), 0, stream,
                       H, x, active, status, gx, gH, gf, glb, gub, d->n, (long long)d->batch, strideH);
  else
    hipLaunchKernelGGL((kkt_bwd_box_dense_kernel<false, true, long long>), dim3((unsigned)blocks), dim3(64), 0, stream,
                       H, x, active, status, gx, gH, gf, glb, gub, d->n, (long long)d->batch, strideH);
  return hipGetLastError();
}

// qpb_solve_box_backward_dual with glam given: the DU forms, plain where H is
// batched (strideH == n n) and SH on one H for the batch (strideH == 0, pass 1
// of the shared form: gH NULL, the sum is pass 2's)
extern "C" hipError_t qpb_launch_kkt_bwd_box_dual(const qpb_desc *d, long long strideH, const double *H,
                                                  const double *x, const uint32_t *active, const int32_t *status,
                                                  const double *gx, const double *glam, double *gH, double *gf,
                                                  double *glb, double *gub, hipStream_t stream) {
  using namespace qpb::bwdbox;
  const bool sh = strideH == 0;
  const long long blocks = (d->batch + QPB - 1) / QPB;
  if (d->n > 16 && sh)
    hipLaunchKernelGGL((kkt_bwd_box_wave_kernel<true, long long, const double *>), dim3((unsigned)d->batch), dim3(64),
                       0, stream, H, x, active, status, gx, gH, gf, glb, gub, d->n, (long long)d->batch, strideH, glam);
  else if (d->n > 16)
    hipLaunchKernelGGL((kkt_bwd_box_wave_kernel<false, const double *>), dim3((unsigned)d->batch), dim3(64), 0, stream,
                       H, x, active, status, gx, gH, gf, glb, gub, d->n, (long long)d->batch, glam);
  else if (d->n == 16 && sh)
    hipLaunchKernelGGL((kkt_bwd_box_dense_kernel<true, true, long long, const double *>), dim3((unsigned)blocks),
                       dim3(64), 0, stream, H, x, active, status, gx, gH, gf, glb, gub, d->n, (long long)d->batch,
                       strideH, glam);
  else if (d->n == 16)
    hipLaunchKernelGGL((kkt_bwd_box_dense_kernel<true, false, const double *>), dim3((unsigned)blocks), dim3(64), 0,
                       stream, H, x, active, status, gx, gH, gf, glb, gub, d->n, (long long)d->batch, glam);
  else if (sh)
    hipLaunchKernelGGL((kkt_bwd_box_dense_kernel<false, true, long long, const double *>), dim3((unsigned)blocks),
                       dim3(64), 0, stream, H, x, active, status, gx, gH, gf, glb, gub, d->n, (long long)d->batch,
                       strideH, glam);
  else
    hipLaunchKernelGGL((kkt_bwd_box_dense_kernel<false, false, const double *>), dim3((unsigned)blocks), dim3(64), 0,
                       stream, H, x, active, status, gx, gH, gf, glb, gub, d->n, (long long)d->batch, glam);
  return hipGetLastError();
}

// qpb_solve_box_backward_multi: the MU forms on H's run-time stride (0 or n n),
// with glam (the DU MU forms) or without; T directions per QP, the right-hand
// sides' QP stride in directions rstride (T, or 0: one set for the batch)
extern "C" hipError_t qpb_launch_kkt_bwd_box_multi(const qpb_desc *d, long long strideH, const double *H,
                                                   const uint32_t *active, const int32_t *status, int T,
                                                   long long rstride, const double *gx, const double *glam,
                                                   double *gf, double *glb, double *gub, hipStream_t stream) {
  using namespace qpb::bwdbox;
  const Multi mu{T, rstride};
  const double *no_x = nullptr;
  double *no_h = nullptr;
  const long long blocks = (d->batch + QPB - 1) / QPB;
  const dim3 grid((unsigned)(d->n > 16 ? d->batch : blocks));
  auto go = [&](auto kernel, auto... tail) {
    hipLaunchKernelGGL(kernel, grid, dim3(64), 0, stream, H, no_x, active, status, gx, no_h, gf, glb, gub, d->n,
                       (long long)d->batch, strideH, tail...);
  };
  if (d->n > 16) {
    if (glam) go(kkt_bwd_box_wave_kernel<true, long long, const double *, Multi>, glam, mu);
    else go(kkt_bwd_box_wave_kernel<true, long long, Multi>, mu);
  } else if (d->n == 16) {
    if (glam) go(kkt_bwd_box_dense_kernel<true, true, long long, const double *, Multi>, glam, mu);
    else go(kkt_bwd_box_dense_kernel<true, true, long long, Multi>, mu);
  } else {
    if (glam) go(kkt_bwd_box_dense_kernel<false, true, long long, const double *, Multi>, glam, mu);
    else go(kkt_bwd_box_dense_kernel<false, true, long long, Multi>, mu);
  }
  return hipGetLastError();
}
