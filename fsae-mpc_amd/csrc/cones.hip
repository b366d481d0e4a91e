// cones.hip -- track corridors from cone positions (the definition is in include/fsaempc.h).  One kernel, beside the
// others: no other unit changes.
//
//   cor_from_cones_kernel   one 256-thread workgroup per corridor:
//     1. the 4M coarse sample points of the spline, s = (j + 0.5) dl / 4, into LDS (once, both sides read them)
//     2. per side: cones strided over the threads -- nearest coarse sample, Newton search, offset along the left normal --, then a
//        bitonic sort in LDS on (s, input index); dropped cones carry the key +inf, the sort is padded to the next power of two
//     3. per side: cells strided over the threads; a binary search finds the last cone at or before the cell, the normal line of
//        the spline is cut with the chord to its cyclic successor
//     4. the thread that wrote a cell's two limits reads them back for the width checks; the counts go through LDS and are summed
//        in thread order, without atomics
// A workgroup reads its own map (or the shared one) and writes its own rows: one corridor's result does not depend on the batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fsaempc.h"
#include "cones.h"
#include "cl_frame.h"

namespace {

constexpr int CONES_T = 256;
enum { CONE_KEPT = 0, CONE_ABSENT = 1, CONE_UNPROJECTED = 2, CONE_STRAY = 3 };

struct ConesLds {                                              // 50 KB
  double cx[4 * FSAEMPC_CONES_MAX_M], cy[4 * FSAEMPC_CONES_MAX_M];   // coarse sample points; the reductions' scratch at the end
  double key[FSAEMPC_CONES_MAX];                               // s of the cones in sorted order (+inf: dropped or padding)
  int idx[FSAEMPC_CONES_MAX];                                  // input index of the cone in that position
  double x[FSAEMPC_CONES_MAX], y[FSAEMPC_CONES_MAX], n[FSAEMPC_CONES_MAX];   // by input index
};

// Stage 2 for one cone: s in [0, L) and the offset n along the unit left normal at the foot point.
__device__ int cone_project(const Spl& sp, double L, double reach, const double* cx, const double* cy, double x0, double y0,
                            double& s_out, double& n_out) {
  if (!(fabs(x0) < INFINITY) || !(fabs(y0) < INFINITY)) return CONE_ABSENT;
  const int n4 = 4 * sp.M;
  double best = INFINITY; int jb = 0;
  for (int j = 0; j < n4; ++j) {                               // (every lane reads the same address: a broadcast)
    const double dx = cx[j] - x0, dy = cy[j] - y0, d2 = dx * dx + dy * dy;
    if (d2 < best) { best = d2; jb = j; }                      // the first minimum in ascending j
  }
  double s = ((double)jb + 0.5) * sp.dl / 4;
  bool done = false;
  for (int it = 0; it < 30 && !done; ++it) {                   // closest_point.m, bounded and guarded
    double X, Xd, Xdd, Y, Yd, Ydd;
    spline3(sp.xP, sp.M, sp.dl, s, X, Xd, Xdd);
    spline3(sp.yP, sp.M, sp.dl, s, Y, Yd, Ydd);
    const double dist_d = 2 * (X - x0) * Xd + 2 * (Y - y0) * Yd;
    const double dist_dd = 2 * (X - x0) * Xdd + 2 * Xd * Xd + 2 * (Y - y0) * Ydd + 2 * Yd * Yd;
    if (!(dist_dd > 0)) return CONE_UNPROJECTED;
    const double delta = dist_d / dist_dd;
    if (!(fabs(delta) <= sp.dl)) return CONE_UNPROJECTED;      // (a NaN step included)
    s = s - delta;
    if (!(fabs(s) < INFINITY)) return CONE_UNPROJECTED;
    done = fabs(delta) <= 1e-10;
  }
  if (!done) return CONE_UNPROJECTED;
  double X, Xd, Xdd, Y, Yd, Ydd;
  spline3(sp.xP, sp.M, sp.dl, s, X, Xd, Xdd);
  spline3(sp.yP, sp.M, sp.dl, s, Y, Yd, Ydd);
  const double nrm = sqrt(Xd * Xd + Yd * Yd);
  const double n = (x0 - X) * (-Yd / nrm) + (y0 - Y) * (Xd / nrm);
  if (!(fabs(n) < INFINITY)) return CONE_UNPROJECTED;
  if (fabs(n) > reach) return CONE_STRAY;
  double r = s - floor(s / L) * L;
  if (!(r >= 0 && r < L)) r = 0.0;                             // (the wrap's own rounding: the point L is the point 0)
  s_out = r; n_out = n;
  return CONE_KEPT;
}

// Stage 3 for one cell of one side with kept >= 2 cones: the edge's offset at s_i; off: the cell lies off its chord.
__device__ double cone_cell_edge(const Spl& sp, double L, const ConesLds& S, int kept, double s_i, bool& off) {
#pragma clang fp contract(off)
  double X, Xd, Xdd, Y, Yd, Ydd;
  spline3(sp.xP, sp.M, sp.dl, s_i, X, Xd, Xdd);
  spline3(sp.yP, sp.M, sp.dl, s_i, Y, Yd, Ydd);
  const double nrm = sqrt(Xd * Xd + Yd * Yd);
  const double Tx = Xd / nrm, Ty = Yd / nrm, Nx = -Yd / nrm, Ny = Xd / nrm;
  int lo = 0, hi = kept;                                       // the last kept cone with s_j <= s_i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (S.key[mid] <= s_i) lo = mid + 1; else hi = mid;
  }
  int j = lo - 1;
  const bool none = j < 0;
  if (none) j = kept - 1;
  const bool last = j + 1 >= kept;
  const int j1 = last ? 0 : j + 1;
  const double sj = none ? S.key[j] - L : S.key[j];
  const double sj1 = none ? S.key[j1] : (last ? S.key[j1] + L : S.key[j1]);
  const int a = S.idx[j], b = S.idx[j1];
  const double cjx = S.x[a], cjy = S.y[a];
  const double dx = S.x[b] - cjx, dy = S.y[b] - cjy;
  const double dT = dx * Tx + dy * Ty;
  double t;
  if (dT > 0) t = ((X - cjx) * Tx + (Y - cjy) * Ty) / dT;
  else t = (s_i - sj) / (sj1 - sj);
  off = !(t >= -1e-9 && t <= 1 + 1e-9);
  t = fmin(fmax(t, 0.0), 1.0);
  return (cjx + t * dx - X) * Nx + (cjy + t * dy - Y) * Ny;
}

__global__ void __launch_bounds__(CONES_T) cor_from_cones_kernel(ConesParams P) {
  __shared__ ConesLds S;
  const int tid = threadIdx.x, cor = blockIdx.x;
  const Spl sp{P.spM, P.spdl, P.xP, P.yP};
  const int n4 = 4 * P.spM;
  for (int j = tid; j < n4; j += CONES_T) {
    const double s = ((double)j + 0.5) * sp.dl / 4;
    double v, d, dd;
    spline3(sp.xP, sp.M, sp.dl, s, v, d, dd); S.cx[j] = v;
    spline3(sp.yP, sp.M, sp.dl, s, v, d, dd); S.cy[j] = v;
  }
  __syncthreads();

  const double ds = P.L / (double)P.N_w;
  int cnt_absent = 0, cnt_unproj = 0, cnt_stray = 0, cnt_off = 0;
  int kept_side[2];
  for (int side = 0; side < 2; ++side) {                       // 0: left (n_hi), 1: right (n_lo); every branch below is uniform
    const int K = side == 0 ? P.n_left : P.n_right;
    const double* cones = side == 0 ? P.left : P.right;
    if (P.per_corridor && K > 0) cones += (size_t)cor * (size_t)K * 2;
    double* out = (side == 0 ? P.n_hi : P.n_lo) + (size_t)cor * (size_t)P.N_w;
    int kept = 0;
    if (K > 0) {
      int n2 = 1;
      while (n2 < K) n2 <<= 1;
      for (int k = tid; k < n2; k += CONES_T) {
        double key = INFINITY;
        if (k < K) {
          const double x0 = cones[2 * (size_t)k], y0 = cones[2 * (size_t)k + 1];
          double s = 0.0, n = 0.0;
          const int st = cone_project(sp, P.L, P.reach, S.cx, S.cy, x0, y0, s, n);
          if (st == CONE_KEPT) key = s;
          else if (st == CONE_ABSENT) ++cnt_absent;
          else if (st == CONE_UNPROJECTED) ++cnt_unproj;
          else ++cnt_stray;
          S.x[k] = x0; S.y[k] = y0; S.n[k] = n;
        }
        S.key[k] = key; S.idx[k] = k;
      }
      __syncthreads();
      for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int i = tid; i < n2; i += CONES_T) {
            const int l = i ^ j;
            if (l > i) {
              const double ki = S.key[i], kl = S.key[l];
              const int ii = S.idx[i], il = S.idx[l];
              const bool gt = ki > kl || (ki == kl && ii > il);
              if (gt == ((i & k) == 0)) { S.key[i] = kl; S.key[l] = ki; S.idx[i] = il; S.idx[l] = ii; }
            }
          }
          __syncthreads();
        }
      }
      int lo = 0, hi = n2;                                     // the kept cones come first: the first +inf key ends them
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (S.key[mid] < INFINITY) lo = mid + 1; else hi = mid;
      }
      kept = lo;
    }
    kept_side[side] = kept;
    const double sgn = side == 0 ? -P.margin : P.margin;
    for (int i = tid; i < P.N_w; i += CONES_T) {
      double e;
      if (kept == 0) e = NAN;
      else if (kept == 1) e = S.n[S.idx[0]];
      else {
        bool off;
        e = cone_cell_edge(sp, P.L, S, kept, (double)i * ds, off);
        if (off) ++cnt_off;
      }
      out[i] = e + sgn;
    }
    __syncthreads();                                           // the next side overwrites the cone arrays
  }
  if (!P.info) return;

  int cnt_bad = 0, cnt_nan = 0;
  double wmin = INFINITY;
  {
    const double* lo = P.n_lo + (size_t)cor * (size_t)P.N_w;
    const double* hi = P.n_hi + (size_t)cor * (size_t)P.N_w;
    for (int i = tid; i < P.N_w; i += CONES_T) {               // the cells this thread wrote
      const double l = lo[i], h = hi[i], w = h - l;
      if (!(l < h)) ++cnt_bad;
      if (!(w == w)) ++cnt_nan; else wmin = fmin(wmin, w);
    }
  }
  int* red = reinterpret_cast<int*>(S.cx);                     // 6 x 256 ints; S.cy: 256 doubles
  red[0 * CONES_T + tid] = cnt_absent; red[1 * CONES_T + tid] = cnt_unproj; red[2 * CONES_T + tid] = cnt_stray;
  red[3 * CONES_T + tid] = cnt_off; red[4 * CONES_T + tid] = cnt_bad; red[5 * CONES_T + tid] = cnt_nan;
  S.cy[tid] = wmin;
  __syncthreads();
  if (tid == 0) {
    int sum[6] = {0, 0, 0, 0, 0, 0};
    double w = INFINITY;
    for (int t = 0; t < CONES_T; ++t) {
      for (int c = 0; c < 6; ++c) sum[c] += red[c * CONES_T + t];
      w = fmin(w, S.cy[t]);
    }
    double* o = P.info + (size_t)cor * FSAEMPC_NCONEINFO;
    o[0] = (double)kept_side[0]; o[1] = (double)kept_side[1];
    o[2] = (double)sum[0]; o[3] = (double)sum[1]; o[4] = (double)sum[2]; o[5] = (double)sum[3]; o[6] = (double)sum[4];
    o[7] = sum[5] > 0 ? NAN : w;
  }
}

}  // namespace

hipError_t cor_from_cones_launch(const ConesParams& P, hipStream_t st) {
  hipLaunchKernelGGL(cor_from_cones_kernel, dim3((unsigned)P.n_corridors), dim3(CONES_T), 0, st, P);
  return hipGetLastError();
}
