// cl_cone_loc.hip -- the cone sensor of the closed loop (no counterpart in main.m, which reads the exact state): range and
// bearing of the nearest detected cones in view of a car, out of the true pose and the true cone map.  The algorithm is stated in
// include/fsaempc.h (fsaempc_cl_cone_sense_batch_device); the scalar rules are those of cl_cone_loc.h.
//
//   cl_cone_sense_kernel   one wavefront per car.  Lane l looks at the cones g = l + 64 t, t = 0 .. 15 (FSAEMPC_CONES_MAX cones per side:
//                          at most 1024 per map), read straight from global memory: view and detection per cone, the true range of a
//                          candidate kept in a register (+inf for everything else; the loop over t is unrolled, so no register array
//                          is indexed by a variable).  The kept set is found in min(seen, k_max) rounds of two wave-wide minima, on
//                          the range and then on the index among the lanes that hold that range (qp_lane.h's wave_min: DPP and lane
//                          swaps, every lane active in every round -- the trip count comes from ballots and is the same in all 64
//                          lanes).  Round k hands its cone to lane k, and lanes 0 .. count - 1 then draw the noise of their cone side by
//                          side.  No atomics, no LDS; a car's result depends on its id, the period and the map only.
#include <hip/hip_runtime.h>
#include <math.h>
#include "cl_cone_loc.h"
#include "qp_lane.h"

namespace {

constexpr int CLC_SLOTS = 2 * FSAEMPC_CONES_MAX / 64;    // cones per lane

__global__ void __launch_bounds__(64) cl_cone_sense_kernel(ClConeSenseParams P) {
  const int lane = threadIdx.x;
  const size_t b = blockIdx.x;                           // (the grid is the batch)
  const int kmax = P.k_max;
  int* ids = P.cone_id + b * (size_t)kmax;
  double* zs = P.cone_z + b * (size_t)kmax * 2;
  if (P.finished && P.finished[b]) {                     // (the whole wavefront: one car) out of the race: nothing is seen
    if (lane < kmax) { ids[lane] = -1; zs[2 * lane] = 0.0; zs[2 * lane + 1] = 0.0; }
    if (lane == 0) { P.cone_n[b] = 0; P.cone_seen[b] = 0; }
    return;
  }
  const double X = P.cart[b * 7], Y = P.cart[b * 7 + 1], psi = P.cart[b * 7 + 2];
  const unsigned long long id = P.id0 + (unsigned long long)b;
  const int ntot = P.truth.n_left + P.truth.n_right;

  double key[CLC_SLOTS];
  int seen = 0;
#pragma unroll
  for (int t = 0; t < CLC_SLOTS; ++t) {
    const int g = lane + 64 * t;
    const bool have = g < ntot;
    double cx, cy, rho, beta;
    clc_cone_at(P.truth, b, have ? g : 0, cx, cy);
    clc_polar(cx, cy, X, Y, psi, rho, beta);
    bool cand = have && clc_in_view(rho, beta, P.r_min, P.r_max, P.fov) != 0;
    if (cand) cand = clc_detected(P.seed, id, P.step, g, P.p_detect) != 0;
    key[t] = cand ? rho : INFINITY;
    seen += __popcll(__ballot(cand));
  }
  seen = __builtin_amdgcn_readfirstlane(seen);
  const int keep = seen < kmax ? seen : kmax;

  int mine = -1;                                         // lane k: the cone of round k
  for (int k = 0; k < keep; ++k) {
    double m = INFINITY; int mt = 0;
#pragma unroll
    for (int t = 0; t < CLC_SLOTS; ++t) { const bool lt = key[t] < m; m = lt ? key[t] : m; mt = lt ? t : mt; }
    const double best = wave_min(m);
    const double gi = (m == best) ? (double)(lane + 64 * mt) : 4096.0;
    const int g = (int)wave_min(gi);
#pragma unroll
    for (int t = 0; t < CLC_SLOTS; ++t) key[t] = (g == lane + 64 * t) ? INFINITY : key[t];
    mine = (lane == k) ? g : mine;
  }

  if (lane < kmax) {
    double rho_m = 0.0, beta_m = 0.0;
    if (lane < keep) {
      double cx, cy, rho, beta;
      clc_cone_at(P.truth, b, mine, cx, cy);
      clc_polar(cx, cy, X, Y, psi, rho, beta);
      clc_detect(P.seed, id, P.step, mine, rho, beta, P.sigma_rho, P.sigma_beta, P.p_detect, rho_m, beta_m);
    }
    ids[lane] = lane < keep ? mine : -1;
    zs[2 * lane] = rho_m; zs[2 * lane + 1] = beta_m;
  }
  if (lane == 0) { P.cone_n[b] = keep; P.cone_seen[b] = seen; }
}

}  // namespace

hipError_t cl_cone_sense_launch(const ClConeSenseParams& P, hipStream_t st) {
  if (P.batch == 0) return hipSuccess;
  hipLaunchKernelGGL(cl_cone_sense_kernel, dim3(P.batch), dim3(64), 0, st, P);
  return hipGetLastError();
}
