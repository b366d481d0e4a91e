// cl_cone_loc.h -- cone-based localisation of the closed loop: what a lidar or a camera at the car's reference point sees
// of the cones of a known map -- range and bearing of the nearest detected cones in view -- and the rows the filter of cl_sensors.hip
// forms from them, written once for the host and the device, and the internal interface between the C ABI and the two kernels
// (cl_cone_sense_kernel in cl_cone_loc.hip, cl_estimate_cones_kernel in cl_sensors.hip).
//
//   cone index        g = 0 .. n_left - 1 the left side, n_left .. n_left + n_right - 1 the right side of an fsaempc_cones map
//   clc_polar         range and bearing of the point (cx, cy) from the pose (X, Y, psi): dx = cx - X, dy = cy - Y,
//                     rho = sqrt(dx dx + dy dy), beta = cls_angdiff(psi, atan2(dy, dx))
//   clc_in_view       r_min <= rho <= r_max and |beta| <= fov / 2 (false for a NaN)
//   clc_detect        the draws of cone g: words of (seed, id, step, 2 + g) -- calls 0 and 1 of that counter layout are the state draws of
//                     cl_latency.h -- detected iff cll_u01(w[2]) < p_detect; rho_m = cll_observe(rho, sigma_rho, z0),
//                     beta_m = cls_angdiff(0, cll_observe(beta, sigma_beta, z1)) (the noisy bearing wrapped to [-pi, pi])
//   clc_before        the order of the selection: the key (rho, g), the true range and then the index
//   clc_select        the min(count, k_max) first candidates in that order (host statement; the kernel finds them by wave-wide minima)
//   clc_rows          the two rows of one observation at the linearisation point: with (h0, h1, h2) = h(x-)[0 .. 2] and Hr the rows and
//                     columns 0 .. 2 of dh/dx(x-): dx = mx - h0, dy = my - h1, q2 = dx dx + dy dy, rho^ = sqrt(q2),
//                     beta^ = cls_angdiff(h2, atan2(dy, dx)), g_rho = (-dx / rho^, -dy / rho^, 0), g_beta = (dy / q2, -dx / q2, -1),
//                     G_i[c] = sum_k g_i[k] Hr[k][c] in the order k = 0, 1, 2, nu0_rho = rho_m - rho^, nu0_beta = cls_angdiff(beta^, beta_m)
//
// The first part compiles as plain C++ (a host program may include this file without the HIP headers).  No FMA contraction in it:
// tests/cone_loc_numpy.py restates every function operation for operation.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "fsaempc.h"
#include "cl_latency.h"
#include "cl_sensors.h"

CLS_HD void clc_polar(double cx, double cy, double X, double Y, double psi, double& rho, double& beta) {
  CLS_NO_CONTRACT
  const double dx = cx - X, dy = cy - Y;
  const double a = dx * dx, b = dy * dy;
  rho = sqrt(a + b);
  beta = cls_angdiff(psi, atan2(dy, dx));
}

CLS_HD int clc_in_view(double rho, double beta, double r_min, double r_max, double fov) {
  CLS_NO_CONTRACT
  return rho >= r_min && rho <= r_max && fabs(beta) <= fov / 2;
}

// returns 1 iff cone g is detected in this period; rho_m and beta_m are written either way
CLS_HD int clc_detect(unsigned long long seed, unsigned long long id, unsigned long long step, int g, double rho, double beta, double sigma_rho,
                      double sigma_beta, double p_detect, double& rho_m, double& beta_m) {
  uint32_t w[4];
  double z[4];
  cll_words(seed, id, step, 2 + g, w);
  cll_normals(w, z);
  rho_m = cll_observe(rho, sigma_rho, z[0]);
  beta_m = cls_angdiff(0.0, cll_observe(beta, sigma_beta, z[1]));
  return cll_u01(w[2]) < p_detect;
}

// the detection alone (the words without the logarithm and the circular functions of the normals)
CLS_HD int clc_detected(unsigned long long seed, unsigned long long id, unsigned long long step, int g, double p_detect) {
  uint32_t w[4];
  cll_words(seed, id, step, 2 + g, w);
  return cll_u01(w[2]) < p_detect;
}

CLS_HD int clc_before(double rho_a, int g_a, double rho_b, int g_b) { return rho_a < rho_b || (rho_a == rho_b && g_a < g_b); }

// rho[g] for g = 0 .. n - 1: the true range of a candidate, anything of a cone that is none (cand[g] == 0).  ids: k_max entries, the
// selection in order, -1 past the count.  Returns the count kept; *seen is the number of candidates.
inline int clc_select(int n, const double* rho, const int* cand, int k_max, int* ids, int* seen) {
  int kept = 0, total = 0;
  for (int k = 0; k < k_max; ++k) ids[k] = -1;
  for (int g = 0; g < n; ++g) total += cand[g] ? 1 : 0;
  for (int k = 0; k < k_max; ++k) {
    int best = -1;
    for (int g = 0; g < n; ++g) {
      if (!cand[g]) continue;
      bool taken = false;
      for (int t = 0; t < kept; ++t) taken = taken || ids[t] == g;
      if (taken) continue;
      if (best < 0 || clc_before(rho[g], g, rho[best], best)) best = g;
    }
    if (best < 0) break;
    ids[kept++] = best;
  }
  *seen = total;
  return kept;
}

// G[0] the range row, G[1] the bearing row (state columns 0 .. 2; the columns >= 3 are zero); nu0 likewise.  rho_hat == 0 leaves
// non-finite entries behind: such a row is not applied
CLS_HD void clc_rows(double h0, double h1, double h2, const double Hr[3][3], double mx, double my, double rho_m, double beta_m, double G[2][3],
                     double nu0[2], double& rho_hat) {
  CLS_NO_CONTRACT
  const double dx = mx - h0, dy = my - h1;
  const double a = dx * dx, b = dy * dy;
  const double q2 = a + b;
  rho_hat = sqrt(q2);
  const double beta_hat = cls_angdiff(h2, atan2(dy, dx));
  const double gr[3] = {-dx / rho_hat, -dy / rho_hat, 0.0};
  const double gb[3] = {dy / q2, -dx / q2, -1.0};
  for (int c = 0; c < 3; ++c) {
    double ar = 0.0, ab = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double pr = gr[k] * Hr[k][c], pb = gb[k] * Hr[k][c];
      ar = ar + pr; ab = ab + pb;
    }
    G[0][c] = ar; G[1][c] = ab;
  }
  nu0[0] = rho_m - rho_hat;
  nu0[1] = cls_angdiff(beta_hat, beta_m);
}

#if defined(__HIPCC__)
struct ClConeMap {                // an fsaempc_cones map on the device
  const double* left; const double* right;   // n_left x 2 / n_right x 2 doubles per map, xy interleaved
  int n_left, n_right;
  int per_car;                    // 0: one map for the batch; 1: one per car, car-major
};
// position of cone g of car b's map (g in range)
__device__ __forceinline__ void clc_cone_at(const ClConeMap& m, size_t b, int g, double& cx, double& cy) {
  const bool lf = g < m.n_left;
  const double* side = lf ? m.left : m.right;
  const size_t n = (size_t)(lf ? m.n_left : m.n_right), i = (size_t)(lf ? g : g - m.n_left);
  const size_t o = ((m.per_car ? b * n : (size_t)0) + i) * 2;
  cx = side[o]; cy = side[o + 1];
}

struct ClConeSenseParams {
  int batch, k_max;
  ClConeMap truth;
  double r_min, r_max, fov, sigma_rho, sigma_beta, p_detect;
  unsigned long long seed, id0, step;
  const double* cart;             // batch x 7
  const int* finished;            // optional
  int* cone_n; int* cone_seen;    // batch each
  int* cone_id;                   // batch x k_max
  double* cone_z;                 // batch x k_max x 2
};
hipError_t cl_cone_sense_launch(const ClConeSenseParams& P, hipStream_t st);

struct ClEstimateConesParams {
  ClEstimateCartParams E;         // everything the Cartesian filter reads and writes
  ClConeMap map;
  int k_max;
  double r_cone[2];               // variances of range and bearing; +inf: the channel is off
  const int* cone_n;              // batch
  const int* cone_id;             // batch x k_max
  const double* cone_z;           // batch x k_max x 2
  double* cone_innov;             // batch x k_max x 2
  int* rows_used;                 // batch
  double* G_out;                  // optional, batch x k_max x 2 x 3
};
// par (optional): the controller's parameter blocks, car b reads par + b * par_stride; null: the constants compiled in
hipError_t cl_estimate_cones_launch(const ClEstimateConesParams& P, hipStream_t st, const double* par = nullptr, int par_stride = 0);
#endif
