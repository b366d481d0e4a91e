// ltv_build_blocked.hip -- QP construction of one LTV-MPC step with move blocking (held inputs), batched, on MI355X (gfx950).
//
// The horizon's N steps are grouped into M blocks of consecutive steps and the input is held over each block: u_k = v_block(k).
// The QP's variables are [v_1 .. v_M; slacks] (nV_b = 2M + ns); its rows stay those of the unblocked problem (nC = 6N / 20N).  With
// E the (2N + ns) x (2M + ns) matrix that copies v_block(k) to step k, the blocked QP is H_b = E'HE, g_b = E'g, A_b = AE of the
// unblocked one (ltv_build.hip); the kernel forms it directly: 2M condensing recursions instead of 2N, nC x nV_b entries of A, a
// SYRK over 2M columns.  The linearisation, the prediction offset, the per-step row coefficients and every row bound do not depend
// on the blocking.  The body is ltv_build_kernel<NX, EXACT, BLK, PAR> of ltv_build_kernel.h, the one ltv_build.hip instantiates
// without blocks; this unit holds its four BLK = true instantiations (kinematic / dynamic, constants compiled in / parameter
// blocks) and their launch, so that the two sets compile side by side.  The block map (at most 98 small integers) travels in the
// kernel arguments.
#include "ltv_build_kernel.h"

hipError_t ltv_build_launch_blocked_unit(const LtvParams& P, const LtvBlockMap& bm, const double* values, int stride, const int* idx,
                                         int batch, hipStream_t st) {
  return select_build<true>(P, &bm, values, stride, idx, batch, st, false);
}
