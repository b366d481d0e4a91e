"""fsaempc for MI355X: the batched LTV-MPC QP hot path of kerry-he/fsae-mpc (linearise -> condense ->
solve) as hand-written gfx950 HIP kernels behind a C ABI (include/fsaempc.h, lib/libfsaempc.so).  This
package is the host-side mirror of the reference's interfaces for that path; it contains no CPU compute path."""
from . import _lib
from ._lib import (CL_MAX_DELAY, CONE_INFO_INDEX, CONE_OBS_MAX, LAP_STATE_INDEX, MAX_LAPS, METRIC_INDEX, NCONEINFO, NLAPSTATE, NMETRIC, NPAR, NREPORT, PARAM_INDEX, REPORT_INDEX, FsaempcError,
                   default_opts, default_params, lib)
from .corridor import Corridor
from .closed_loop import CartesianSensors, ClosedLoop, ConeSensor, Estimator, LapReport, Latency, Nmpc, cl_noise, monte_carlo, monte_carlo_carts, nmpc_accept, nmpc_shift
from .ltvmpc import LtvBatch, dims, ltvmpc_dynamic_curvilinear, ltvmpc_kinetmatic_curvilinear
from .plan import Plan, raceline_qp
from .qpoases import qp_layout, qp_solve_batch_device, qpOASES, qpOASES_sequence
from .sqp import SqpBatch, sqp_timing
from .sensitivity import (LtvStepFunction, QpFunction, feedback_gain, ltv_step_affine_maps, ltv_step_diff, ltv_step_lambda,
                          ltv_step_vjp, qp_vjp)
from .reference import obtain_reference, obtain_reference_batch_device, reference_live_batch_device
from .synthetic import DYNAMIC, KINEMATIC, cone_draws, instances, param_draws, reference_live
from .tracks import Track

__all__ = ["FsaempcError", "default_opts", "lib", "LtvBatch", "dims", "ltvmpc_dynamic_curvilinear",
           "ltvmpc_kinetmatic_curvilinear", "qp_solve_batch_device", "qpOASES", "qpOASES_sequence", "DYNAMIC", "KINEMATIC",
           "instances", "reference_live", "Track", "obtain_reference", "obtain_reference_batch_device",
           "reference_live_batch_device", "ClosedLoop", "monte_carlo", "monte_carlo_carts", "SqpBatch", "sqp_timing", "QpFunction", "qp_vjp",
           "LtvStepFunction", "feedback_gain", "ltv_step_affine_maps", "ltv_step_diff", "ltv_step_lambda", "ltv_step_vjp", "NPAR", "PARAM_INDEX", "default_params", "param_draws", "qp_layout", "Plan", "raceline_qp",
           "LapReport", "METRIC_INDEX", "NMETRIC", "REPORT_INDEX", "NREPORT", "Corridor",
           "LAP_STATE_INDEX", "NLAPSTATE", "MAX_LAPS", "CONE_INFO_INDEX", "NCONEINFO", "cone_draws",
           "Latency", "cl_noise", "CL_MAX_DELAY", "Estimator", "Nmpc", "nmpc_shift", "nmpc_accept", "CartesianSensors", "ConeSensor", "CONE_OBS_MAX"]
