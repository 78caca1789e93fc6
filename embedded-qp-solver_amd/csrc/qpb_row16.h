// qpb_row16.h -- what the kernels that map one QP onto a 16-lane DPP row, four
// QPs per wavefront, have in common: the LDS slot of a QP and the steps around
// it.  Internal; device code, and the host's choice among the kernels' forms.
// Used by qpb_gi.hip (gi_dense), qpb_gi_box.hip (gi_box) and qpb_kkt_bwd.hip
// (kkt_bwd_dense_kernel).  `l` is the lane's index 0..15 in its row throughout.
//
// These kernels are hand-scheduled, and a step is here only in a form that
// leaves every caller's listing as it was, instruction for instruction and
// register for register (tools/asm_same.py against the build before; the record
// of the first round is profiles/row16/).  The compiler's early passes see a
// function's body apart from its caller's, so not every form does: where a
// whole loop in a function moved a listing, the function is one step of it and
// the loop stays with the caller (back_subst_step, rotate_pair, h_padded).
#pragma once

#include "qpb_common.h"

namespace qpb {
namespace row16 {

constexpr int NL = 16;  // lanes per QP
constexpr int QPB = 4;  // QPs per workgroup (one wavefront)
constexpr int RS = 18;  // row stride (doubles) of the input transposes: conflict-free b128

// packed lower triangle of L (lrow).  Reads may run past a row's end into the
// next rows (always inside the QP's slot): the solves never use those values.
constexpr int L_SIZE = lrow(NL);  // 136

// LDS slot of one QP: 394 doubles = 3,152 B, 12,608 B per wave -> 12 waves
// per CU (3 per SIMD, matching the VGPR budget).  A CU holds 12 one-wave
// workgroups of up to 12,800 B of LDS each and 11 from 13,056 B
// (tools/probe/occupancy_probe.hip, measured on the MI355X): the round-4 slot
// (426 doubles, 13,632 B per wave) ran 11 waves per CU, one SIMD in four
// with two (the wave timeline, tools/wave_timeline.py).
constexpr int OFF_L = 0;                  // L (136)
constexpr int OFF_R = L_SIZE;             // R, column-major 16 x 16 with a zero diagonal: R[i][j] at
                                          // j*16 + i; column 0 (no entry above the diagonal, never read
                                          // by the back substitution) doubles as the exchange row
constexpr int OFF_XCH = OFF_R + NL * NL;  // 392: the exchange's two scalars (s_p, |d|^2)
constexpr int SLOT = OFF_XCH + 2;         // 394
static_assert(SLOT % 2 == 0 && OFF_R % 2 == 0 && OFF_XCH % 2 == 0, "b128 alignment");
static_assert(QPB * SLOT * 8 <= kWaveLdsMax, "12 waves (3 per SIMD) per CU by LDS");
static_assert(NL * RS <= SLOT, "input transposes are staged over the whole slot");

// The slot of the wave's QP `slot`, in the order 0, 2, 1, 3: ds_read_b64 serves
// 32 lanes (two QPs) per cycle; slots 0/1 and 2/3 are 2 SLOT = 788 doubles
// apart, 40 banks mod 64, so contiguous 16-lane reads of the two QPs share 8
// of the 64 banks (one slot apart they would share 20)
__device__ __forceinline__ double *slot_base(double *lds, int slot) {
  return lds + (((slot & 1) << 1) | (slot >> 1)) * SLOT;
}

// The QP of row `slot` of workgroup `block`, for the kernels that index by QP.
// Rows past the end of the batch (last group only) do not leave: they replay
// the batch's last QP -- same trip count, so they never extend the wave's
// loop -- and store nothing (!live).  Every lane of the wave stays live, so the
// cross-row reads (wave_max4's readlanes) only ever see real QP state.
struct RaggedQp {
  bool live;
  long long g;
};
__device__ __forceinline__ RaggedQp ragged_qp(unsigned block, int slot, long long batch) {
  const long long graw = (long long)block * QPB + slot;
  const bool live = graw < batch;
  return {live, live ? graw : batch - 1};
}

// Entry j of row l of the n x n matrix Hq, n < 16, padded with the identity
// outside n (lc = min(l, n - 1): every load is in bounds)
__device__ __forceinline__ double h_padded(const double *Hq, int l, int lc, int n, int j) {
  const double h = Hq[lc * n + (j < n ? j : n - 1)];
  return (l < n && j < n) ? h : (l == j ? 1.0 : 0.0);
}

// L -> LDS, packed rows (lane l writes row l), kept for the final solves.
// Lane l also writes its dead entries j > l, over the start of later rows:
// stores go in descending j, and a row's own entry at such an address has
// a smaller j, so it lands last (a wave's DS instructions execute in order).
__device__ __forceinline__ void store_l(double *Lp, int l, const double (&Lr)[NL]) {
  unroll<NL>([&](auto J) {
    constexpr int j = NL - 1 - J;
    Lp[lrow(l) + j] = Lr[j];
    wave_lds_sync();
  });
}

// Step J of the lane-parallel back substitution over R's columns, J = 15 .. 1
// in that order (column 0 holds no entry above the diagonal), behind its
// wave-uniform test J < qmax.  On the negated accumulator: nacc_l += R[l][J] r_J
// with r_J = nacc_J ninv_J, ninv = -1 / R_JJ, read from lane J by the FMA
// itself; the product was written just before, so fmac_bc_nop issues the DPP
// read hazard's wait states.
template <int J>
__device__ __forceinline__ void back_subst_step(const double *R, int l, int qmax, double &nacc, double ninv) {
  if (J > 0 && J < qmax) fmac_bc_nop<J>(nacc, nacc * ninv, R[J * NL + l]);
}

// ---- in a DROP ------------------------------------------------------------------
// Givens rotation J (c, s) on columns J, J + 1 of a row of D.  The callers read
// (c, s) from lane J by DPP moves (bc<J>), not by a fused operand: no hazard
// contract here.
template <int J>
__device__ __forceinline__ void rotate_pair(double (&row)[NL], double cj, double sj) {
  const double e0 = row[J], e1 = row[J + 1];
  row[J] = __builtin_fma(cj, e0, sj * e1);
  row[J + 1] = __builtin_fma(-sj, e0, cj * e1);
}

// Back to the zero-diagonal form: returns R[l][l] (0 for l >= q) and zeroes it
__device__ __forceinline__ double take_diagonal(double *R, int l, int q) {
  wave_lds_sync();
  const double dg = (l < q) ? R[l * NL + l] : 0.0;
  wave_lds_sync();
  if (l < q) R[l * NL + l] = 0.0;
  return dg;
}

// ---- after the loop -------------------------------------------------------------
// x_l from g = f + A^T lam: L y = g, L^T x = -y, lane-parallel: step k
// broadcasts the finished component from lane k (a DPP move of a product the
// compiler schedules: no hazard contract); finished lanes keep updating (dead
// values) and the components are captured by same-address LDS stores in
// xcap (16).  Lrow: row l of L (entries past l are dead), invd = 1 / L[l][l].
// Used by gi_box and kkt_bwd_box; gi_dense runs solve_x_frozen below, the same
// arithmetic without the capture.
__device__ __forceinline__ double solve_x(double gl, double invd, const double (&Lrow)[NL], const double *Lp, int l,
                                          double *xcap) {
  {
    double acc = gl;
    unroll<NL>([&](auto K) {
      constexpr int kk = K;
      const double yk = bc<kk>(acc * invd);
      acc = __builtin_fma(-Lrow[kk], yk, acc);
      xcap[kk] = yk;
    });
  }
  wave_lds_sync();
  {
    double acc = xcap[l];
    wave_lds_sync();
    unroll<NL>([&](auto K) {
      constexpr int kk = NL - 1 - K;
      const double xk = bc<kk>(acc * invd);
      acc = __builtin_fma(-Lp[lrow(kk) + l], xk, acc);
      xcap[kk] = xk;
    });
  }
  wave_lds_sync();
  return -xcap[l];
}

// solve_x without the capture (gi_dense): a finished lane is frozen by EXEC
// instead.  One step under the lanes l >= K (FWD) or l <= K of every row:
// t = acc invd, acc -= t_K mul, the same product and the same fused
// multiply-add on the same numbers as solve_x's step K (t_K read from lane K
// by the FMA itself, two wait states after its product; the multiplier's sign
// by the source modifier).  A lane leaves the mask after its own step, so its
// t stays the finished component: no broadcast move, no LDS store.  All 64
// lanes must be live on entry (the callers run one wavefront per workgroup
// and call this outside divergent code; -DQPB_CHECK_EXEC traps where that does
// not hold); EXEC is all ones again on exit, and
// it changes only inside the one asm statement, where the compiler places
// nothing.
template <int K, bool FWD>
__device__ __forceinline__ void frozen_step(double &acc, double &t, double invd, double mul) {
  constexpr unsigned m16 = FWD ? (0xFFFFu << K) & 0xFFFFu : 0xFFFFu >> (NL - 1 - K);
  asm volatile("s_mov_b32 exec_lo, %4\n\ts_mov_b32 exec_hi, %4\n\t"
               "v_mul_f64 %1, %0, %2\n\ts_nop 1\n\t"
               "v_fmac_f64_dpp %0, %1, -%3 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
               "s_mov_b64 exec, -1"
               : "+v"(acc), "+v"(t)
               : "v"(invd), "v"(mul), "i"(m16 * 0x10001u), "i"(K));
}
// x_l as solve_x returns it, bit for bit: L y = g forward, then L^T x = -y
// backward from the y each lane kept
__device__ __forceinline__ double solve_x_frozen(double gl, double invd, const double (&Lrow)[NL], const double *Lp,
                                                 int l) {
#ifdef QPB_CHECK_EXEC
  // diagnostic build: the precondition of frozen_step, all 64 lanes live
  if (__builtin_amdgcn_read_exec() != ~0ull) __builtin_trap();
#endif
  double acc = gl, y = 0.0, x = 0.0;
  unroll<NL>([&](auto K) { frozen_step<K, true>(acc, y, invd, Lrow[K]); });
  acc = y;
  unroll<NL>([&](auto K) {
    constexpr int kk = NL - 1 - K;
    frozen_step<kk, false>(acc, x, invd, Lp[lrow(kk) + l]);
  });
  return -x;
}

// a non-finite x on any lane -> QPB_NUMERICAL for a QP that was QPB_OK
__device__ __forceinline__ int x_status(int status, double xl) {
  const double bad = row_min((__builtin_fabs(xl) < kInf) ? 0.0 : -1.0);
  return (status == QPB_OK && bad < 0.0) ? QPB_NUMERICAL : status;
}

// ---- host: the kernel form for (n, m) ---------------------------------------------
// f(MR, N16, FULL), integral constants.  MR: rows per lane (m <= 16 MR).
// N16: n == 16 (coalesced loads).  FULL: n == 16 and m == 16 MR (no padding
// rows: no masking anywhere).
template <class F>
inline void dispatch_form(int n, int m, F &&f) {
  using std::bool_constant;
  using std::integral_constant;
  const bool n16 = n == 16;
  if (m <= 16) {
    if (n16 && m == 16) f(integral_constant<int, 1>{}, bool_constant<true>{}, bool_constant<true>{});
    else if (n16) f(integral_constant<int, 1>{}, bool_constant<true>{}, bool_constant<false>{});
    else f(integral_constant<int, 1>{}, bool_constant<false>{}, bool_constant<false>{});
  } else {
    if (n16 && m == 32) f(integral_constant<int, 2>{}, bool_constant<true>{}, bool_constant<true>{});
    else if (n16) f(integral_constant<int, 2>{}, bool_constant<true>{}, bool_constant<false>{});
    else f(integral_constant<int, 2>{}, bool_constant<false>{}, bool_constant<false>{});
  }
}

}  // namespace row16
}  // namespace qpb
