// qpb_kkt_bwd_sum.hip -- pass 2 of qpb_solve_shared_backward for gfx950: the
// gradient of an H or an A that the whole batch shares is the sum over the
// batch of the per-QP gradients,
//
//     gH = 1/2 (S + S^T),  S = DX^T X                  (n x B times B x n)
//     gA = DL^T X + LM^T DX                            (m x B times B x n)
//
// with row k of X, DX, DL, LM the x, dx, dlam and masked lam of QP k: DX = gf
// and DL = -gb as pass 1 (qpb_kkt_bwd.hip) wrote them, LM = lam where the row's
// bit is set.  A QP whose status is not QPB_OK contributes exactly 0: its four
// rows are SELECTED to 0.0, never multiplied by 0, so a NaN in its x or lam
// meets nothing; lam outside the active set is dropped the same way.
//
// These are tall-skinny GEMMs with K = the QP index, on the fp64 matrix cores.
// kkt_bwd_sum_kernel: one wave per slice of the batch (qpb::sum_plan, a
// function of the batch size alone), four QPs per v_mfma_f64_16x16x4_f64: lane
// l feeds a = dx[k0 + (l >> 4)][16 ti + (l & 15)] and
// b = x[k0 + (l >> 4)][16 tj + (l & 15)] (the operand layout of qpb_gen.hip),
// tiles of 16 x 16: ceil(n/16)^2 for S and ceil(m/16) ceil(n/16) for gA, at most
// 4 + 8 tiles = 96 accumulator VGPRs.  Lanes past n, m or the slice's end feed
// 0.0.  At n = 16 a load of x or gf is 512 contiguous bytes.  The wave writes
// its tiles to its slot of the workspace.
// kkt_bwd_sum_finish_kernel: sixteen threads per output element add the slots,
// each its own in slot order and then the sixteen partial sums in order, and
// write gH[i][j] = 0.5 (S[i][j] + S[j][i]) -- one commutative add of the same
// two sums for (i, j) and (j, i), so gH is symmetric bit for bit -- and gA.
// No atomics: the bits of the sums are a function of the inputs and of
// (n, m, batch) only, whatever the stream, the workspace's history or the
// number of CUs.
#include <type_traits>

#include "qpb_launch.h"  // with qpb.h
#include "qpb_route.h"   // sum_plan, sum_slot_doubles

namespace qpb {
namespace bwd {

using d4 = __attribute__((__vector_size__(4 * sizeof(double)))) double;
constexpr int kSumUnroll = 4;  // matrix-core steps (of 4 QPs) whose loads a wave has in flight

// NT = ceil(n / 16); MT = ceil(m / 16), or 0 when gA is not wanted.  The slot
// holds S as a (16 NT) x (16 NT) row-major matrix, then gA's sum as
// (16 MT) x (16 NT); parts that are not wanted are not written (nor read).
// BX (empty, or one int: pass 2 of qpb_solve_range_box_backward): the row stride
// ms of lam and of the mask words' rows.  It is m everywhere else; in this form
// m is mg, the rows of G that are summed, gbg is pass 1's unrouted B x mg array
// and lam and active keep the mg + n rows of the solve: a row < mg feeds the
// numbers the call on [G; I] feeds for it, and an output element of the
// matrix-core instruction depends on its own row and column only.
template <int NT, int MT, class... BX>
__global__ __launch_bounds__(64) void kkt_bwd_sum_kernel(
    const double *__restrict__ xg, const double *__restrict__ dxg, const double *__restrict__ gbg,
    const double *__restrict__ lamg, const uint32_t *__restrict__ actg, const int32_t *__restrict__ statg,
    double *__restrict__ slots, int n, int m, long long batch, long long per, long long slot_doubles, int wantH,
    BX... msg) {
  static_assert(std::is_same_v<void(BX...), void()> || std::is_same_v<void(BX...), void(int)>);
  int ms = m;
  if constexpr (sizeof...(BX) == 1) ms = (msg, ...);
  const int l = threadIdx.x, c = l & 15, q = l >> 4;
  const long long kb = (long long)blockIdx.x * per;  // < batch: the plan has no empty slice
  const long long ke = kb + per < batch ? kb + per : batch;
  constexpr int MTA = MT > 0 ? MT : 1;
  d4 S[NT][NT], G[MTA][NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) S[i][j] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < MTA; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) G[i][j] = d4{0.0, 0.0, 0.0, 0.0};
  const int words = (ms + 31) / 32;
  // kSumUnroll steps of 4 QPs per trip: every load of the trip is issued before
  // its first matrix-core instruction, so a wave has kSumUnroll steps' loads in
  // flight instead of one (one step per trip waited a full memory latency per
  // step).  Steps past the slice's end feed zeros.
  for (long long k0 = kb; k0 < ke; k0 += 4 * kSumUnroll) {
    double xa[kSumUnroll][NT], da[kSumUnroll][NT], dl[kSumUnroll][MTA], lm[kSumUnroll][MTA];
#pragma unroll
    for (int u = 0; u < kSumUnroll; ++u) {
      // the lane's QP; past the slice's end the loads read the slice's last QP
      // and the values are dropped
      const long long k = k0 + 4 * u + q;
      const bool valid = k < ke;
      const long long kc = valid ? k : ke - 1;
      const bool ok = valid && (statg ? statg[kc] == QPB_OK : true);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int col = 16 * t + c;
        const bool in = col < n;
        const long long e = kc * n + (in ? col : 0);
        const double xv = xg[e], dv = dxg[e];
        xa[u][t] = (ok && in) ? xv : 0.0;
        da[u][t] = (ok && in) ? dv : 0.0;
      }
      if constexpr (MT > 0) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const int row = 16 * t + c;
          const bool in = row < m;
          const int rc = in ? row : 0;
          const double gbv = gbg[kc * m + rc], lv = lamg[kc * ms + rc];
          const uint32_t w = actg[kc * words + (rc >> 5)];
          const bool bit = (w >> (rc & 31)) & 1u;
          dl[u][t] = (ok && in) ? -gbv : 0.0;
          lm[u][t] = (ok && in && bit) ? lv : 0.0;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kSumUnroll; ++u) {
      if (wantH) {
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            S[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(da[u][i], xa[u][j], S[i][j], 0, 0, 0);
      }
      if constexpr (MT > 0) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            G[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(dl[u][i], xa[u][j], G[i][j], 0, 0, 0);
            G[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(lm[u][i], da[u][j], G[i][j], 0, 0, 0);
          }
      }
    }
  }
  // C/D layout: column l & 15, rows (l >> 4) + 4 r
  double *o = slots + (long long)blockIdx.x * slot_doubles;
  constexpr int LD = 16 * NT;
  if (wantH) {
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[(16 * i + q + 4 * r) * LD + 16 * j + c] = S[i][j][r];
  }
  if constexpr (MT > 0) {
    double *oa = o + LD * LD;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) oa[(16 * i + q + 4 * r) * LD + 16 * j + c] = G[i][j][r];
  }
}

// One output element per 16 threads: thread p of them adds the slots p, p + 16,
// ... in that order (independent loads, several in flight), the 16 partial sums
// are added in the order of p by the first of them.  Element e < n n is gH's,
// n n + e is gA's; ld = 16 ceil(n/16).  A workgroup of 256 threads takes 16
// consecutive elements, thread t element t & 15 of them with p = t >> 4.
constexpr int kFinParts = 16;
__global__ __launch_bounds__(256) void kkt_bwd_sum_finish_kernel(const double *__restrict__ slots, long long nslots,
                                                                 long long slot_doubles, int ld, int n, int m,
                                                                 double *__restrict__ gH, double *__restrict__ gA) {
  __shared__ double pa[kFinParts][16], pb[kFinParts][16];
  const int t = threadIdx.x, le = t & 15, p = t >> 4;
  const int e = (int)blockIdx.x * 16 + le;
  const int nn = n * n, total = nn + m * n;
  const bool isH = e < nn;
  const bool live = e < total && (isH ? gH != nullptr : gA != nullptr);
  double a = 0.0, b = 0.0;
  if (live) {
    const int ea = isH ? e : e - nn;
    const int i = ea / n, j = ea - i * n;
    // gH: S[i][j] and S[j][i]; gA: its element (the second sum reads it again and is not used)
    const double *pij = slots + (isH ? 0 : ld * ld) + i * ld + j;
    const double *pji = isH ? slots + j * ld + i : pij;
#pragma unroll 8
    for (long long s = p; s < nslots; s += kFinParts) {
      a += pij[s * slot_doubles];
      b += pji[s * slot_doubles];
    }
  }
  pa[p][le] = a;
  pb[p][le] = b;
  __syncthreads();
  if (p == 0 && live) {
    double sa = pa[0][le], sb = pb[0][le];
#pragma unroll
    for (int r = 1; r < kFinParts; ++r) {
      sa += pa[r][le];
      sb += pb[r][le];
    }
    // (i, j) and (j, i) add the same two sums: symmetric bit for bit
    if (isH) gH[e] = 0.5 * (sa + sb);
    else gA[e - nn] = sa;
  }
}

}  // namespace bwd
}  // namespace qpb

// gH, gA: the n x n and m x n sums, either may be NULL (not both); dx = pass 1's
// gf, gb pass 1's (read for gA only).  slots: sum_plan(batch).slots times
// sum_slot_doubles(n, m) doubles of scratch.  The whole batch in one launch.
extern "C" hipError_t qpb_launch_kkt_bwd_sum(const qpb_desc *d, const double *x, const double *dx, const double *gb,
                                             const double *lam, const uint32_t *active, const int32_t *status,
                                             double *slots, double *gH, double *gA, hipStream_t stream) {
  const qpb::SumPlan plan = qpb::sum_plan(d->batch);
  const long long sd = qpb::sum_slot_doubles(d->n, d->m);
  const int nt = (d->n + 15) / 16, mt = gA ? (d->m + 15) / 16 : 0;
  auto launch = [&](auto NT, auto MT) {
    hipLaunchKernelGGL((qpb::bwd::kkt_bwd_sum_kernel<NT(), MT()>), dim3((unsigned)plan.slots), dim3(64), 0, stream, x,
                       dx, gb, lam, active, status, slots, d->n, d->m, (long long)d->batch, plan.per, sd,
                       gH ? 1 : 0);
  };
  auto with_nt = [&](auto MT) {
    if (nt == 1) launch(std::integral_constant<int, 1>{}, MT);
    else launch(std::integral_constant<int, 2>{}, MT);
  };
  switch (mt) {
    case 0: with_nt(std::integral_constant<int, 0>{}); break;
    case 1: with_nt(std::integral_constant<int, 1>{}); break;
    case 2: with_nt(std::integral_constant<int, 2>{}); break;
    case 3: with_nt(std::integral_constant<int, 3>{}); break;
    default: with_nt(std::integral_constant<int, 4>{}); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int elems = d->n * d->n + d->m * d->n;
  hipLaunchKernelGGL(qpb::bwd::kkt_bwd_sum_finish_kernel, dim3((unsigned)((elems + 15) / 16)), dim3(256), 0, stream,
                     slots, plan.slots, sd, 16 * nt, d->n, d->m, gH, gA);
  return hipGetLastError();
}

// pass 2 of qpb_solve_range_box_backward: the same two launches over the mg rows
// of G (d->m is mg + n), from pass 1's gf (dx) and its unrouted gbw
extern "C" hipError_t qpb_launch_kkt_bwd_sum_range_box(const qpb_desc *d, int mg, const double *x, const double *dx,
                                                       const double *gbw, const double *lam, const uint32_t *active,
                                                       const int32_t *status, double *slots, double *gH, double *gG,
                                                       hipStream_t stream) {
  const qpb::SumPlan plan = qpb::sum_plan(d->batch);
  const long long sd = qpb::sum_slot_doubles(d->n, mg);
  const int nt = (d->n + 15) / 16, mt = gG ? (mg + 15) / 16 : 0;
  auto launch = [&](auto NT, auto MT) {
    hipLaunchKernelGGL((qpb::bwd::kkt_bwd_sum_kernel<NT(), MT(), int>), dim3((unsigned)plan.slots), dim3(64), 0,
                       stream, x, dx, gbw, lam, active, status, slots, d->n, mg, (long long)d->batch, plan.per, sd,
                       gH ? 1 : 0, (int)d->m);
  };
  auto with_nt = [&](auto MT) {
    if (nt == 1) launch(std::integral_constant<int, 1>{}, MT);
    else launch(std::integral_constant<int, 2>{}, MT);
  };
  // (mg + n <= 64 with n >= 1: at most 4 row tiles, as above)
  switch (mt) {
    case 0: with_nt(std::integral_constant<int, 0>{}); break;
    case 1: with_nt(std::integral_constant<int, 1>{}); break;
    case 2: with_nt(std::integral_constant<int, 2>{}); break;
    case 3: with_nt(std::integral_constant<int, 3>{}); break;
    default: with_nt(std::integral_constant<int, 4>{}); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int elems = d->n * d->n + mg * d->n;
  hipLaunchKernelGGL(qpb::bwd::kkt_bwd_sum_finish_kernel, dim3((unsigned)((elems + 15) / 16)), dim3(256), 0, stream,
                     slots, plan.slots, sd, 16 * nt, d->n, mg, gH, gG);
  return hipGetLastError();
}
