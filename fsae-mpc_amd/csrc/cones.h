// cones.h -- track corridors from cone positions: the internal interface between the C ABI and cones.hip.
//
// Per corridor and side the kernel projects every cone onto the track spline (nearest of 4M coarse samples, then the Newton search of
// spline/closest_point.m on cl_frame.h's spline3), orders the kept cones by (s, input index) and, per cell of the corridor's tables,
// cuts the normal line of the spline at s_i with the chord between the two cones that bracket s_i.  The tables have the layout
// corridor.h's CorTable reads; include/fsaempc.h states the definition, tests/cones_numpy.py restates it.
#pragma once
#include <hip/hip_runtime.h>
#include "fsaempc.h"

struct ConesParams {
  int spM; double spdl; const double* xP; const double* yP;   // the track spline (device)
  double L;
  const double* left; const double* right;                     // n_left x 2 / n_right x 2 doubles per map, xy interleaved
  int n_left, n_right;
  int per_corridor;                                            // 0: one map for all corridors
  int n_corridors, N_w;
  double margin, reach;
  double* n_lo; double* n_hi;                                  // n_corridors x N_w each
  double* info;                                                // n_corridors x FSAEMPC_NCONEINFO, or NULL
};
// one 256-thread workgroup per corridor; about 50 KB of static LDS
hipError_t cor_from_cones_launch(const ConesParams& P, hipStream_t st);
