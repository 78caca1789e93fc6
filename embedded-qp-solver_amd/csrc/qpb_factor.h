// qpb_factor.h -- the layout of a factor buffer (qpb_factor_shared ->
// qpb_solve_factored): what one shared H and A turn into once, so that a solve
// starts from L and D = A L^-T instead of computing them per QP.  Plain C++
// without a HIP header: the host compiler builds it alone, the factor kernels
// (which write a buffer) and the factored solve forms (which read it) share it.
//
// A buffer is self-contained -- the solve takes neither H nor A -- and belongs
// to one (n, m): the kernel class, and with it the layout, follows from the
// shape exactly as the route does.  All offsets are in doubles.
//
//   header (kHdr)   [0] what the set-up found that does not depend on b: 0,
//                   QPB_NOT_SPD or QPB_NUMERICAL (a row of A with a NaN entry or
//                   a non-finite squared norm), as a double; [1] n; [2] m;
//                   [3] 16 or 32, the padded n of the class
//   L               the Cholesky factor of H, padded as the class's kernel pads it
//   D               A L^-T, one row per lane as the class's kernel holds it
//   an2, an, dn2    per row |a_r|^2, |a_r| = |a_r|^2 rsqrt(|a_r|^2) (the value the
//                   unfactored kernel forms its threshold from) and |D_r|^2
//   A               the caller's A, row-major m x n (the x recovery re-reads the
//                   active rows)
//
// L and D are stored for the solve kernels' loads: a load instruction's lanes
// read consecutive addresses.
//   n <= 16, m <= 32 (gi_dense: lane l of a QP's 16 holds row l of L and rows
//   l + 16 r of D, r < MR):
//     L   [t][l][c], t < 8, c < 2: L[l][2t + c] -- one 16-byte load per lane and
//         t, the 16 lanes read 256 contiguous bytes; 16 x 16, the identity
//         outside n
//     D   [r][t][l][c]: D[l + 16 r][2t + c], rows >= m and columns >= n zero
//     an2, an, dn2   [r][l]
//   otherwise, n <= 32, m <= 64 (gi_wave: lane l of 64 holds row l of D):
//     L   packed rows, L[i][j] at i (i + 1) / 2 + j, 32 rows (zero from row n
//         on): copied flat into the kernel's LDS, element i 64 + l by lane l
//     D   [t][l][c], t < 16, c < 2: D[l][2t + c] -- the 64 lanes read 1 KiB
//     an2, an, dn2   [l]
#pragma once

namespace qpb {
namespace fct {

constexpr int kHdr = 8;
constexpr int kMaxN = 32, kMaxM = 64;  // the limit of qpb_factor_shared and qpb_solve_factored

struct Layout {
  bool dense;     // the n <= 16, m <= 32 class
  int mr;         // dense: rows of D per lane
  long long L;    // offsets
  long long D, an2, an, dn2, A;
  long long size;  // doubles in all
};

constexpr Layout layout(int n, int m) {
  Layout y{};
  y.dense = n <= 16 && m <= 32;
  y.mr = m <= 16 ? 1 : 2;
  const long long lsize = y.dense ? 256 : 32 * 33 / 2;
  const long long rows = y.dense ? 16LL * y.mr : 64, cols = y.dense ? 16 : 32;
  y.L = kHdr;
  y.D = y.L + lsize;
  y.an2 = y.D + rows * cols;
  y.an = y.an2 + rows;
  y.dn2 = y.an + rows;
  y.A = y.dn2 + rows;
  y.size = y.A + (long long)m * n;
  return y;
}

static_assert(layout(16, 32).dense && layout(16, 32).mr == 2 && !layout(16, 33).dense && !layout(17, 0).dense);
static_assert(layout(16, 32).size == 8 + 256 + 512 + 96 + 512 && layout(1, 0).size == 8 + 256 + 256 + 48);
static_assert(layout(32, 64).size == 8 + 528 + 2048 + 192 + 2048);
// every section starts on a 16-byte boundary (the b128 loads of L and D)
static_assert(layout(16, 32).D % 2 == 0 && layout(16, 32).L % 2 == 0 && layout(32, 64).D % 2 == 0 &&
              layout(7, 5).D % 2 == 0 && layout(20, 3).D % 2 == 0);

}  // namespace fct

// The backward's buffer (qpb_factor_shared_backward -> qpb_solve_factored_backward),
// a layout of its own: it is written by the backward kernels' own set-up
// (qpb_kkt_bwd.hip), so that what remains per QP is the unfactored kernel's
// operations on the unfactored kernel's numbers, and it holds neither A nor the
// row norms -- no output of the backward reads them.  One (n, m), one class,
// offsets in doubles, as above.
//
//   header (kHdr)   [0] 0 or QPB_NOT_SPD (a pivot that was not a positive finite
//                   number), as a double; [1] n; [2] m; [3] 16 or 32
//   n <= 16, m <= 32 (kkt_bwd_dense_kernel: lane l of a QP's 16 holds row l of L
//   and rows l + 16 r of D, r < MR):
//     L    the packed lower triangle as store_l leaves it in the LDS slot, 136
//          doubles, zero up to kDenseL: 16-byte piece t 16 + l by lane l, t < 5
//     ik   [k]: 1 / L_kk, the sweep's ik of step k = the kernel's invLd of lane k
//     nc   [t][l][c], t < 8, c < 2: the multiplier nc of lane l at step 2t + c of
//          the u recursion
//     D    [r][t][l][c]: the lane's E[r][2t + c] after the sweep; rows >= m and
//          columns >= n zero
//   otherwise, n <= 32, m <= 64 (kkt_bwd_wave_kernel: lane j < 32 holds component j):
//     L    the kernel's 32 x 33 LDS image after the factorisation, padding
//          included (the rows' 33rd words zero): a flat copy
//     ik   [j]: 1 / L_jj, 1 on the padding (the kernel's invLd of lane j)
//     D    [r][j], r < m: row r of A L^-T by the kernel's forward substitution
namespace bfct {

constexpr int kHdr = fct::kHdr;
constexpr int kMaxN = fct::kMaxN, kMaxM = fct::kMaxM;
constexpr int kDenseL = 160;           // 136 rounded up to a 16-byte piece per lane and load
constexpr int kWaveL = 32 * 33;        // WN * WS of qpb_kkt_bwd.hip

struct Layout {
  bool dense;  // the n <= 16, m <= 32 class
  int mr;      // dense: rows of D per lane
  long long L, ik, nc, D;  // offsets (nc: dense only)
  long long size;          // doubles in all
};

constexpr Layout layout(int n, int m) {
  Layout y{};
  y.dense = n <= 16 && m <= 32;
  y.mr = m <= 16 ? 1 : 2;
  y.L = kHdr;
  y.ik = y.L + (y.dense ? kDenseL : kWaveL);
  y.nc = y.ik + (y.dense ? 16 : 32);
  y.D = y.nc + (y.dense ? 256 : 0);
  y.size = y.D + (y.dense ? 256LL * y.mr : 32LL * m);
  return y;
}

static_assert(layout(16, 32).dense && layout(16, 32).mr == 2 && !layout(16, 33).dense && !layout(17, 0).dense);
static_assert(layout(16, 32).dense == fct::layout(16, 32).dense && layout(16, 33).dense == fct::layout(16, 33).dense &&
              layout(17, 0).dense == fct::layout(17, 0).dense);
static_assert(layout(16, 32).size == 8 + 160 + 16 + 256 + 512 && layout(1, 0).size == 8 + 160 + 16 + 256 + 256);
static_assert(layout(32, 64).size == 8 + 1056 + 32 + 2048 && layout(17, 0).size == 8 + 1056 + 32 &&
              layout(16, 33).size == 8 + 1056 + 32 + 33 * 32);
// every section starts on a 16-byte boundary (the b128 loads and copies)
static_assert(layout(16, 32).L % 2 == 0 && layout(16, 32).ik % 2 == 0 && layout(16, 32).nc % 2 == 0 &&
              layout(16, 32).D % 2 == 0 && layout(7, 5).D % 2 == 0 && layout(7, 5).size % 2 == 0);
static_assert(layout(32, 64).L % 2 == 0 && layout(32, 64).ik % 2 == 0 && layout(32, 64).D % 2 == 0 &&
              layout(20, 3).D % 2 == 0 && layout(20, 3).size % 2 == 0);
static_assert(kDenseL % 32 == 0 && kDenseL >= 16 * 17 / 2 && kWaveL % 2 == 0);

}  // namespace bfct

// The box solve's buffer (qpb_factor_box -> qpb_solve_box_factored), a third
// layout: A = [I; -I] is implicit, so D = [L^-T; -L^-T] is stored once, as the
// rows of L^-T, and the box recovery x = -H^-1 (f + lam_u - lam_l) reads
// neither H nor A -- the buffer holds neither.  It belongs to one n; the class
// follows from n alone, as qpb_solve_box's does.  Offsets in doubles.
//
//   header (kHdr)   [0] 0 or QPB_NOT_SPD, as a double; [1] n; [2] 16 or 32, the
//                   padded n of the class
//   n <= 16 (gi_box: lane l of a QP's 16 holds row l of L and row l of L^-T):
//     L    [t][l][c], t < 8, c < 2: L[l][2t + c] -- one 16-byte load per lane and
//          t, the 16 lanes read 256 contiguous bytes; 16 x 16, the identity
//          outside n, zero right of the diagonal
//     D    [t][l][c]: row l of L^-T, entry 2t + c (the lower bound's row is its
//          negative)
//     dn2  [l]: |row l|^2, what the unfactored kernel starts fn2 from
//   16 < n <= 32 (gi_wave's BOX form: lane l < n holds row l of L^-T, lane n + i
//   its negated row i):
//     L    packed rows, L[i][j] at i (i + 1) / 2 + j, 32 rows (zero from row n
//          on): copied flat into the kernel's LDS, element i 64 + l by lane l
//     D    [t][r][c], t < 16, r < 32, c < 2: row r of L^-T, entry 2t + c, zero
//          from row n on -- a lane's load is 16 bytes, lanes 0 .. n-1 and
//          n .. 2n-1 each read consecutive addresses
//     dn2  [r]: |row r|^2, what the unfactored kernel starts dn from; zero from
//          row n on
namespace bxfct {

constexpr int kHdr = fct::kHdr;
constexpr int kMaxN = 32;  // the limit of qpb_factor_box and qpb_solve_box_factored

struct Layout {
  bool box16;            // the n <= 16 class
  int np;                // the padded n: 16 or 32
  long long L, D, dn2;   // offsets
  long long size;        // doubles in all
};

constexpr Layout layout(int n) {
  Layout y{};
  y.box16 = n <= 16;
  y.np = y.box16 ? 16 : 32;
  y.L = kHdr;
  y.D = y.L + (y.box16 ? 256 : 32 * 33 / 2);
  y.dn2 = y.D + (long long)y.np * y.np;
  y.size = y.dn2 + y.np;
  return y;
}

static_assert(layout(1).box16 && layout(16).box16 && !layout(17).box16 && !layout(32).box16);
static_assert(layout(1).size == 8 + 256 + 256 + 16 && layout(16).size == layout(1).size);
static_assert(layout(17).size == 8 + 528 + 1024 + 32 && layout(32).size == layout(17).size);
// the class boundary is the general buffer's at m = 2n
static_assert(layout(16).box16 == fct::layout(16, 32).dense && layout(17).box16 == fct::layout(17, 34).dense);
// every section starts on a 16-byte boundary (the b128 loads of L and D), and so does the end
static_assert(layout(16).L % 2 == 0 && layout(16).D % 2 == 0 && layout(16).dn2 % 2 == 0 && layout(16).size % 2 == 0);
static_assert(layout(32).L % 2 == 0 && layout(32).D % 2 == 0 && layout(32).dn2 % 2 == 0 && layout(32).size % 2 == 0);
// no H and no A: smaller than the general buffer of the explicit A = [I; -I]
static_assert(layout(16).size < fct::layout(16, 32).size && layout(32).size < fct::layout(32, 64).size);

}  // namespace bxfct
}  // namespace qpb
