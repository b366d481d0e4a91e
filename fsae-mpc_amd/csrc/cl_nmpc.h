// cl_nmpc.h -- internal interface between the C ABI and the kernels of cl_nmpc.hip: the batched SQP as the controller of the closed
// loop.  Plan shift into the SQP's start, the skip mask of the SQP, take-over of its result.
#pragma once
#include <hip/hip_runtime.h>

// u_init[b, k] = u_keep[b, k + 1] (k < N - 1), u_init[b, N - 1] = u_keep[b, N - 1]; shift == 0: a copy.  skip[b] = finished[b] != 0
// (finished null: 0).  u_init must not overlap u_keep (the C ABI refuses it).
hipError_t cl_nmpc_shift_launch(int N, int batch, int shift, const double* u_keep, const int* finished, double* u_init, int* skip, hipStream_t st);

// status[i] = FSAEMPC_SQP_SKIPPED where skip[i] != 0; runs between sqp_init_launch and the first compaction.
hipError_t sqp_skip_launch(int batch, const int* skip, int* status, hipStream_t st);

// len_x = nx N, len_u = 2 N entries per car; qp_iter and skip may be null.
hipError_t cl_nmpc_accept_launch(int len_x, int len_u, int batch, const double* x_new, const double* u_new, const int* status, const int* qp_iter,
                                 const int* skip, double* x_keep, double* u_keep, int* exitflag, int* iter, hipStream_t st);
