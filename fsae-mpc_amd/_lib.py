"""ctypes binding of libfsaempc.so (include/fsaempc.h).  The library is HIP-only: there is no CPU
fallback anywhere in this package -- if the .so is missing or no gfx950 device is present the calls
raise."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FSAEMPC_LIB") or os.path.join(_HERE, "lib", "libfsaempc.so")

EXPORTS = [
    "fsaempc_qp_default_opts", "fsaempc_qp_workspace_bytes", "fsaempc_qp_solve_batch_device", "fsaempc_qp_solve_batch",
    "fsaempc_ltv_nx", "fsaempc_ltv_nV", "fsaempc_ltv_nC", "fsaempc_ltv_build_qp_batch_device",
    "fsaempc_ltv_workspace_bytes", "fsaempc_ltv_step_batch_device", "fsaempc_ltv_step_batch_device_aux", "fsaempc_last_error", "fsaempc_selftest_mfma", "fsaempc_selftest_lane_reduce", "fsaempc_selftest_diag_factor", "fsaempc_selftest_initial_point",
    "fsaempc_debug_set_dump", "fsaempc_qp_solve_batch_device_aux", "fsaempc_qp_set_timing", "fsaempc_qp_get_timing", "fsaempc_ltv_get_timing",
    "fsaempc_seq_init", "fsaempc_seq_hotstart", "fsaempc_seq_hotstart_matrices", "fsaempc_seq_equality", "fsaempc_seq_cleanup",
    "fsaempc_obtain_reference_batch_device", "fsaempc_reference_live_batch_device",
    "fsaempc_cl_pre_batch_device", "fsaempc_cl_plant_batch_device", "fsaempc_cl_accept_batch_device",
    "fsaempc_track_from_csv", "fsaempc_track_from_points", "fsaempc_track_free", "fsaempc_track_save", "fsaempc_track_load", "fsaempc_track_last_error",
    "fsaempc_nlp_build_qp_batch_device", "fsaempc_sqp_default_opts", "fsaempc_sqp_workspace_bytes", "fsaempc_sqp_batch_device",
    "fsaempc_sqp_get_timing", "fsaempc_qp_vjp_workspace_bytes", "fsaempc_qp_vjp_batch_device",
    "fsaempc_ltv_affine_maps_batch_device", "fsaempc_ltv_step_batch_device_lambda", "fsaempc_ltv_step_vjp_workspace_bytes",
    "fsaempc_ltv_step_vjp_batch_device",
    "fsaempc_ltv_default_params", "fsaempc_ltv_build_qp_batch_device_p", "fsaempc_ltv_step_batch_device_p",
    "fsaempc_nlp_build_qp_batch_device_p", "fsaempc_sqp_batch_device_p", "fsaempc_cl_plant_batch_device_p",
    "fsaempc_ltv_blocked_nV", "fsaempc_ltv_build_qp_batch_device_b", "fsaempc_ltv_workspace_bytes_b", "fsaempc_ltv_step_batch_device_b",
    "fsaempc_qp_workspace_bytes_s", "fsaempc_qp_solve_batch_device_s", "fsaempc_qp_layout",
    "fsaempc_plan_profile_batch_device", "fsaempc_plan_reference_batch_device", "fsaempc_cl_pre_plan_batch_device",
    "fsaempc_raceline_build_qp_device", "fsaempc_plan_line_profile_batch_device", "fsaempc_plan_raceline_workspace_bytes",
    "fsaempc_plan_raceline_batch_device",
    "fsaempc_cl_metrics_batch_device", "fsaempc_cl_report",
    "fsaempc_ltv_build_qp_batch_device_c", "fsaempc_ltv_step_batch_device_c", "fsaempc_cl_metrics_batch_device_c",
    "fsaempc_plan_raceline_batch_device_c", "fsaempc_corridor_line_bounds_device",
    "fsaempc_cl_lap_gate_batch_device", "fsaempc_cl_lap_summary",
    "fsaempc_plan_raceline_cells_workspace_bytes", "fsaempc_plan_raceline_cells_batch_device", "fsaempc_corridor_line_rows_device",
    "fsaempc_corridor_from_cones_device", "fsaempc_track_cones_from_csv", "fsaempc_track_cones_free",
    "fsaempc_plan_line_lapgrad_batch_device", "fsaempc_plan_minlap_workspace_bytes", "fsaempc_plan_minlap_batch_device",
    "fsaempc_cl_noise_batch_device", "fsaempc_cl_observe_batch_device", "fsaempc_cl_history_slot",
    "fsaempc_cl_estimate_batch_device",
    "fsaempc_cl_sense_batch_device", "fsaempc_cl_estimate_cart_batch_device",
    "fsaempc_cl_cone_sense_batch_device", "fsaempc_cl_estimate_cones_batch_device",
    "fsaempc_sqp_batch_device_m", "fsaempc_cl_nmpc_shift_batch_device", "fsaempc_cl_nmpc_accept_batch_device",
]

# fsaempc_ltv_params blocks (include/fsaempc.h FSAEMPC_P_*; tests check this table against the header's macros)
NPAR = 32
PARAM_INDEX = {name: i for i, name in enumerate(
    ["M", "IZ", "LF", "LR", "GRAV", "PB", "PC", "PD", "PE", "Q_S", "Q_N", "Q_MU", "Q_TERMINAL", "R_ACC", "R_STEER",
     "R_SOFT0", "R_SOFT1", "R_SOFT2", "R_SOFT3", "U_ACC_MAX", "U_STEER_MAX", "DELTA_MAX", "N_MAX", "V_MIN", "ALAT_MAX", "SLIP_MAX",
     "ELL_LONG", "ELL_LAT", "PID_KP_V", "PID_MAX_F", "PID_KP_D", "PID_MAX_DRATE"])}

# per-car records of the lap report (include/fsaempc.h FSAEMPC_M_*) and its batch summary (FSAEMPC_R_*); tests check both tables
# against the header's macros
NMETRIC = 16
METRIC_INDEX = {name: i for i, name in enumerate(
    ["STEPS", "STATUS", "N_VIOL_INT", "N_VIOL_MAX", "N_ABS_MAX", "ABNORMAL", "OBJ_SUM", "OBJ_CNT", "SLACK_N_CNT", "SLACK_TYRE_CNT",
     "ELL_VIOL_INT", "ELL_VIOL_MAX", "ITER_SUM", "ITER_MAX", "S_START", "S_LAST"])}
NREPORT = 20
REPORT_INDEX = {name: i for i, name in enumerate(
    ["CARS_DRIVING", "CARS_FINISHED", "CARS_LOST", "LAP_MEAN", "LAP_MIN", "LAP_MAX", "STEPS", "ABNORMAL_PCT", "SLACK_N_PCT", "SLACK_TYRE_PCT",
     "OBJ_MEAN", "N_VIOL_INT_MEAN", "N_VIOL_INT_MAX", "N_VIOL_MAX", "ELL_VIOL_INT_MEAN", "ELL_VIOL_INT_MAX", "ELL_VIOL_MAX", "ITER_MEAN",
     "ITER_MAX", "N_ABS_MAX"])}
# per-car state of the lap gate (include/fsaempc.h FSAEMPC_LS_*; tests check the table against the header's macros)
MAX_LAPS = 64
NLAPSTATE = 4
LAP_STATE_INDEX = {name: i for i, name in enumerate(["DONE", "STEPS", "S_PREV", "T_CROSS"])}


CL_MAX_DELAY = 4     # FSAEMPC_CL_MAX_DELAY
SQP_SKIPPED = 4      # FSAEMPC_SQP_SKIPPED


def check_laps(laps):
    """Validates a lap count (no library call) and returns it as an int."""
    if isinstance(laps, bool) or int(laps) != laps:
        raise ValueError("laps must be an integer")
    if not 1 <= int(laps) <= MAX_LAPS:
        raise ValueError("laps must be 1 .. %d" % MAX_LAPS)
    return int(laps)


class QpOpts(C.Structure):
    _fields_ = [("tol", C.c_double), ("tol_loose", C.c_double), ("tol_x", C.c_double), ("inf_bound", C.c_double),
                ("max_iter", C.c_int), ("polish", C.c_int)]


class QpAux(C.Structure):
    _fields_ = [("kkt", C.c_void_p), ("polished", C.c_void_p), ("x_init", C.c_void_p), ("difficulty", C.c_void_p)]


class QpDesc(C.Structure):
    _fields_ = [("nV", C.c_int), ("nC", C.c_int), ("batch", C.c_int), ("shared_HA", C.c_int)]


class QpVjpIO(C.Structure):
    _fields_ = [("xbar", C.c_void_p), ("fbar", C.c_void_p), ("gbar", C.c_void_p), ("lbbar", C.c_void_p), ("ubbar", C.c_void_p),
                ("lbAbar", C.c_void_p), ("ubAbar", C.c_void_p), ("Hbar", C.c_void_p), ("Abar", C.c_void_p)]


class LtvVjpIO(C.Structure):
    _fields_ = [("ubar", C.c_void_p), ("xbar", C.c_void_p), ("sbar", C.c_void_p), ("fbar", C.c_void_p), ("x0bar", C.c_void_p),
                ("xrefbar", C.c_void_p)]


class Spline(C.Structure):
    _fields_ = [("M", C.c_int), ("dl", C.c_double), ("xP", C.c_void_p), ("yP", C.c_void_p)]


class LtvDesc(C.Structure):
    _fields_ = [("model", C.c_int), ("N", C.c_int), ("batch", C.c_int), ("dt", C.c_double), ("integrator", C.c_int)]


class LtvParams(C.Structure):
    _fields_ = [("values", C.c_void_p), ("per_instance", C.c_int)]


class ClLatency(C.Structure):   # fsaempc_cl_latency
    _fields_ = [("delay", C.c_int), ("compensate", C.c_int), ("sigma", C.c_void_p), ("sigma_per_instance", C.c_int),
                ("seed", C.c_ulonglong), ("id0", C.c_longlong)]


class ClEstimator(C.Structure):   # fsaempc_cl_estimator
    _fields_ = [("q", C.c_void_p), ("q_per_instance", C.c_int), ("r", C.c_void_p), ("r_per_instance", C.c_int), ("p0", C.c_void_p), ("L", C.c_double)]


class ClSensors(C.Structure):   # fsaempc_cl_sensors
    _fields_ = [("sigma", C.c_void_p), ("sigma_per_instance", C.c_int), ("seed", C.c_ulonglong), ("id0", C.c_longlong)]


CONE_OBS_MAX = 16    # FSAEMPC_CONE_OBS_MAX


class LtvBlocking(C.Structure):
    _fields_ = [("n_blocks", C.c_int), ("len", C.POINTER(C.c_int))]


PLAN_MAX_NS = 4096   # FSAEMPC_PLAN_MAX_NS
LINE_MAX_NS = 2048   # FSAEMPC_LINE_MAX_NS
LINE_MIN_NC = 8      # FSAEMPC_LINE_MIN_NC
MAX_NV = 196         # FSAEMPC_MAX_NV
MINLAP_MAX_NS = 1024   # FSAEMPC_MINLAP_MAX_NS
MINLAP_MAX_RHO = 16    # FSAEMPC_MINLAP_MAX_RHO
MINLAP_RHO = (1e4, 3e3, 1e3, 300.0, 100.0, 30.0, 10.0, 3.0)   # the default ladder of Plan.minlap


class PlanTable(C.Structure):   # fsaempc_plan
    _fields_ = [("table", C.c_void_p), ("t", C.c_void_p), ("N_s", C.c_int), ("ds", C.c_double), ("per_instance", C.c_int)]


class CorridorTable(C.Structure):   # fsaempc_corridor
    _fields_ = [("n_lo", C.c_void_p), ("n_hi", C.c_void_p), ("N_w", C.c_int), ("ds", C.c_double), ("per_instance", C.c_int)]


NCONEINFO = 8        # FSAEMPC_NCONEINFO
CONES_MAX = 512      # FSAEMPC_CONES_MAX
CONES_MAX_M = 512    # FSAEMPC_CONES_MAX_M
CONE_INFO_INDEX = {name: i for i, name in enumerate(
    ["KEPT_LEFT", "KEPT_RIGHT", "ABSENT", "UNPROJECTED", "BEYOND_REACH", "CELLS_OFF_SEGMENT", "CELLS_NO_ROOM", "WIDTH_MIN"])}


class ConeMaps(C.Structure):   # fsaempc_cones
    _fields_ = [("left", C.c_void_p), ("right", C.c_void_p), ("n_left", C.c_int), ("n_right", C.c_int), ("per_corridor", C.c_int)]


class ClConeSensor(C.Structure):   # fsaempc_cl_cone_sensor
    _fields_ = [("truth", C.POINTER(ConeMaps)), ("r_min", C.c_double), ("r_max", C.c_double), ("fov", C.c_double), ("sigma_range", C.c_double),
                ("sigma_bearing", C.c_double), ("p_detect", C.c_double), ("k_max", C.c_int), ("seed", C.c_ulonglong), ("id0", C.c_longlong)]


def check_blocking(blocking, N):
    """Validates a sequence of block lengths for a horizon of N steps (no library call) and returns it as a list of ints."""
    try:
        lens = [int(v) for v in blocking]
    except TypeError:
        raise ValueError("blocking must be a sequence of block lengths")
    if any(int(v) != v for v in blocking):
        raise ValueError("blocking: the block lengths must be integers")
    if len(lens) < 1:
        raise ValueError("blocking: at least one block")
    if min(lens) < 1:
        raise ValueError("blocking: every block length must be >= 1")
    if sum(lens) != N:
        raise ValueError("blocking: the block lengths sum to %d, the horizon has N = %d steps" % (sum(lens), N))
    return lens


class Blocking:
    """A validated move blocking and the fsaempc_ltv_blocking that points at its (host) length array."""

    def __init__(self, blocking, N):
        self.lens = check_blocking(blocking, N)
        self.n_blocks = len(self.lens)
        self.trivial = self.n_blocks == N
        self._arr = (C.c_int * self.n_blocks)(*self.lens)
        self.c = LtvBlocking(self.n_blocks, C.cast(self._arr, C.POINTER(C.c_int)))
        self.block_of_step = [j for j, l in enumerate(self.lens) for _ in range(l)]
        self.start = [sum(self.lens[:j]) for j in range(self.n_blocks)]

    def ref(self):
        return C.byref(self.c)


class SqpOpts(C.Structure):
    _fields_ = [("max_sweeps", C.c_int), ("trials", C.c_int), ("tol_step", C.c_double), ("tol_feas", C.c_double), ("armijo", C.c_double),
                ("rho0", C.c_double), ("warm_start", C.c_int)]


class SqpAux(C.Structure):
    _fields_ = [("lambda_", C.c_void_p), ("qp_iter", C.c_void_p), ("step_norm", C.c_void_p), ("hard_viol", C.c_void_p), ("merit", C.c_void_p)]


class TrackTable(C.Structure):
    _fields_ = [("M", C.c_int), ("dl", C.c_double), ("L", C.c_double), ("xP", C.POINTER(C.c_double)), ("yP", C.POINTER(C.c_double))]


class FsaempcError(RuntimeError):
    pass


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise FsaempcError("libfsaempc.so not built (%s): run `make` or __graft_entry__.build(); "
                               "there is no CPU fallback" % LIB_PATH)
        try:                       # the library and torch must share ONE HIP runtime: torch ships its own libamdhip64, and a process
            import torch  # noqa: F401  that binds /opt/rocm's copy first and torch's afterwards ends up with a runtime that sees no device
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.fsaempc_last_error.restype = C.c_char_p
        L.fsaempc_qp_workspace_bytes.restype = C.c_longlong
        L.fsaempc_ltv_workspace_bytes.restype = C.c_longlong
        L.fsaempc_sqp_workspace_bytes.restype = C.c_longlong
        L.fsaempc_qp_vjp_workspace_bytes.restype = C.c_longlong
        L.fsaempc_ltv_step_vjp_workspace_bytes.restype = C.c_longlong
        vp, ll = C.c_void_p, C.c_longlong
        L.fsaempc_qp_solve_batch_device.argtypes = [C.POINTER(QpDesc)] + [vp] * 7 + [C.POINTER(QpOpts)] + [vp] * 5 + [vp, ll, vp]
        L.fsaempc_qp_solve_batch_device_aux.argtypes = [C.POINTER(QpDesc)] + [vp] * 7 + [C.POINTER(QpOpts)] + [vp] * 5 + [C.POINTER(QpAux), vp, ll, vp]
        L.fsaempc_qp_vjp_workspace_bytes.argtypes = [C.POINTER(QpDesc)]
        L.fsaempc_qp_vjp_batch_device.argtypes = [C.POINTER(QpDesc), C.c_int] + [vp] * 7 + [vp] * 4 + [C.POINTER(QpOpts), C.POINTER(QpVjpIO), vp, vp, ll, vp]
        L.fsaempc_ltv_affine_maps_batch_device.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline)] + [vp] * 5
        L.fsaempc_ltv_step_batch_device_lambda.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline)] + [vp] * 4 + [C.POINTER(QpOpts)] + [vp] * 7 + \
            [C.POINTER(QpAux), vp, ll, vp]
        L.fsaempc_ltv_step_vjp_workspace_bytes.argtypes = [C.POINTER(LtvDesc), C.c_int]
        L.fsaempc_ltv_step_vjp_batch_device.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.c_int] + [vp] * 4 + [vp] * 5 + \
            [C.POINTER(QpOpts), C.POINTER(LtvVjpIO), vp, vp, ll, vp]
        L.fsaempc_qp_solve_batch.argtypes = [C.POINTER(QpDesc)] + [vp] * 7 + [C.POINTER(QpOpts)] + [vp] * 5
        L.fsaempc_ltv_build_qp_batch_device.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline)] + [vp] * 4 + [vp] * 7 + [vp] * 3 + [vp]
        L.fsaempc_ltv_step_batch_device.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline)] + [vp] * 4 + [C.POINTER(QpOpts)] + [vp] * 6 + [vp, ll, vp]
        L.fsaempc_ltv_step_batch_device_aux.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline)] + [vp] * 4 + [C.POINTER(QpOpts)] + [vp] * 6 + [C.POINTER(QpAux), vp, ll, vp]
        L.fsaempc_nlp_build_qp_batch_device.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline)] + [vp] * 3 + [vp] * 7 + [vp] * 3 + [vp]
        L.fsaempc_sqp_default_opts.argtypes = [C.POINTER(SqpOpts)]
        L.fsaempc_sqp_workspace_bytes.argtypes = [C.POINTER(LtvDesc)]
        L.fsaempc_sqp_batch_device.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline)] + [vp] * 3 + [C.POINTER(QpOpts), C.POINTER(SqpOpts)] + \
            [vp] * 6 + [C.POINTER(SqpAux), vp, ll, vp]
        L.fsaempc_sqp_get_timing.argtypes = [C.POINTER(C.c_double)] * 4
        L.fsaempc_obtain_reference_batch_device.argtypes = [vp, C.c_double, C.c_int, vp, vp, C.c_double, C.c_int, C.c_int, vp, vp]
        L.fsaempc_reference_live_batch_device.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, vp, vp, vp]
        L.fsaempc_cl_pre_batch_device.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(Spline), vp, vp, C.c_int, vp, vp, vp, vp]
        L.fsaempc_cl_plant_batch_device.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, vp, vp, vp, vp, vp, vp, vp]
        L.fsaempc_cl_accept_batch_device.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
        L.fsaempc_ltv_default_params.argtypes = [C.c_int, C.POINTER(C.c_double)]
        L.fsaempc_ltv_build_qp_batch_device_p.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams)] + [vp] * 4 + [vp] * 7 + [vp] * 3 + [vp]
        L.fsaempc_ltv_step_batch_device_p.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams)] + [vp] * 4 + [C.POINTER(QpOpts)] + \
            [vp] * 7 + [C.POINTER(QpAux), vp, ll, vp]
        L.fsaempc_nlp_build_qp_batch_device_p.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams)] + [vp] * 3 + [vp] * 7 + [vp] * 3 + [vp]
        L.fsaempc_sqp_batch_device_p.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams)] + [vp] * 3 + \
            [C.POINTER(QpOpts), C.POINTER(SqpOpts)] + [vp] * 6 + [C.POINTER(SqpAux), vp, ll, vp]
        L.fsaempc_cl_plant_batch_device_p.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(LtvParams), vp, vp, vp, vp, vp, vp, vp]
        L.fsaempc_ltv_blocked_nV.argtypes = [C.c_int, C.POINTER(LtvBlocking)]
        L.fsaempc_ltv_build_qp_batch_device_b.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams), C.POINTER(LtvBlocking)] + \
            [vp] * 4 + [vp] * 7 + [vp] * 3 + [vp]
        L.fsaempc_ltv_workspace_bytes_b.restype = C.c_longlong
        L.fsaempc_ltv_workspace_bytes_b.argtypes = [C.POINTER(LtvDesc), C.POINTER(LtvBlocking)]
        L.fsaempc_ltv_step_batch_device_b.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams), C.POINTER(LtvBlocking)] + \
            [vp] * 4 + [C.POINTER(QpOpts)] + [vp] * 7 + [C.POINTER(QpAux), vp, ll, vp]
        L.fsaempc_qp_workspace_bytes_s.restype = C.c_longlong
        L.fsaempc_qp_workspace_bytes_s.argtypes = [C.POINTER(QpDesc), C.c_int]
        L.fsaempc_qp_solve_batch_device_s.argtypes = [C.POINTER(QpDesc), C.c_int] + [vp] * 7 + [C.POINTER(QpOpts)] + [vp] * 5 + \
            [C.POINTER(QpAux), vp, ll, vp]
        L.fsaempc_qp_layout.argtypes = [C.POINTER(QpDesc), C.c_int, C.POINTER(C.c_int)]
        L.fsaempc_plan_profile_batch_device.argtypes = [C.c_int, C.POINTER(Spline), C.c_double, C.POINTER(LtvParams), C.c_int, C.c_int,
                                                        C.c_double, C.c_double, vp, vp, vp]
        L.fsaempc_plan_reference_batch_device.argtypes = [C.c_int, C.POINTER(PlanTable), vp, C.c_double, C.c_int, C.c_int, vp, vp]
        L.fsaempc_cl_pre_plan_batch_device.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(Spline), C.POINTER(PlanTable),
                                                       vp, vp, C.c_int, vp, vp, vp, vp]
        L.fsaempc_raceline_build_qp_device.argtypes = [C.POINTER(Spline), C.c_double, C.c_int, C.c_int, vp, vp, vp]
        L.fsaempc_plan_line_profile_batch_device.argtypes = [C.c_int, C.POINTER(Spline), C.c_double, C.POINTER(LtvParams), C.c_int, C.c_int, C.c_int,
                                                             vp, C.c_int, C.c_double, C.c_double, vp, vp, vp]
        L.fsaempc_plan_raceline_workspace_bytes.restype = C.c_longlong
        L.fsaempc_plan_raceline_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.fsaempc_plan_raceline_batch_device.argtypes = [C.c_int, C.POINTER(Spline), C.c_double, C.POINTER(LtvParams), C.c_int, C.c_int, C.c_int,
                                                         C.c_double, C.c_double, C.c_double, C.POINTER(QpOpts), vp, vp, vp, vp, vp, ll, vp]
        L.fsaempc_cl_metrics_batch_device.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(LtvParams)] + [vp] * 10
        L.fsaempc_cl_report.argtypes = [vp, C.c_int, C.c_double, vp]
        L.fsaempc_ltv_build_qp_batch_device_c.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams), C.POINTER(LtvBlocking),
                                                          C.POINTER(CorridorTable)] + [vp] * 4 + [vp] * 7 + [vp] * 3 + [vp]
        L.fsaempc_ltv_step_batch_device_c.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams), C.POINTER(LtvBlocking),
                                                      C.POINTER(CorridorTable)] + [vp] * 4 + [C.POINTER(QpOpts)] + [vp] * 7 + [C.POINTER(QpAux), vp, ll, vp]
        L.fsaempc_cl_metrics_batch_device_c.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(LtvParams),
                                                        C.POINTER(CorridorTable)] + [vp] * 10
        L.fsaempc_corridor_line_bounds_device.argtypes = [C.POINTER(CorridorTable), C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp]
        L.fsaempc_plan_raceline_batch_device_c.argtypes = [C.c_int, C.POINTER(Spline), C.c_double, C.POINTER(LtvParams), C.POINTER(CorridorTable),
                                                           C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(QpOpts),
                                                           vp, vp, vp, vp, vp, ll, vp]
        L.fsaempc_plan_raceline_cells_workspace_bytes.restype = C.c_longlong
        L.fsaempc_plan_raceline_cells_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.fsaempc_plan_raceline_cells_batch_device.argtypes = [C.c_int, C.POINTER(Spline), C.c_double, C.POINTER(LtvParams), C.POINTER(CorridorTable),
                                                               C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(QpOpts),
                                                               vp, vp, vp, vp, vp, vp, ll, vp]
        L.fsaempc_corridor_line_rows_device.argtypes = [C.POINTER(CorridorTable), C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp]
        L.fsaempc_corridor_from_cones_device.argtypes = [C.POINTER(Spline), C.c_double, C.POINTER(ConeMaps), C.c_int, C.c_int, C.c_double, C.c_double,
                                                         vp, vp, vp, vp]
        L.fsaempc_track_cones_from_csv.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_int),
                                                   C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_int)]
        L.fsaempc_plan_line_lapgrad_batch_device.argtypes = [C.c_int, C.POINTER(Spline), C.c_double, C.POINTER(LtvParams), C.c_int, C.c_int, C.c_int,
                                                             vp, C.c_int, C.c_double, C.c_double, vp, vp, vp]
        L.fsaempc_plan_minlap_workspace_bytes.restype = C.c_longlong
        L.fsaempc_plan_minlap_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.fsaempc_plan_minlap_batch_device.argtypes = [C.c_int, C.POINTER(Spline), C.c_double, C.POINTER(LtvParams), C.c_int, C.c_int, C.c_int,
                                                       C.c_double, C.c_double, C.c_double, C.POINTER(QpOpts), C.c_int, C.POINTER(C.c_double), C.c_int,
                                                       vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ll, vp]
        L.fsaempc_track_cones_free.argtypes = [C.POINTER(C.c_double)]
        L.fsaempc_track_cones_free.restype = None
        L.fsaempc_cl_lap_gate_batch_device.argtypes =[C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int] + [vp] * 9
        L.fsaempc_cl_lap_summary.argtypes = [vp, C.c_int, C.c_int, vp]
        L.fsaempc_cl_noise_batch_device.argtypes = [C.c_int, C.c_int, C.c_ulonglong, ll, ll, vp, vp]
        L.fsaempc_cl_observe_batch_device.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams), C.POINTER(ClLatency), ll] + [vp] * 6
        L.fsaempc_cl_history_slot.argtypes = [C.c_int, ll, C.c_int]
        L.fsaempc_cl_estimate_batch_device.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams), C.POINTER(ClEstimator),
                                                       vp, vp, vp, ll] + [vp] * 10
        L.fsaempc_cl_sense_batch_device.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(ClSensors), ll] + [vp] * 7
        L.fsaempc_cl_estimate_cart_batch_device.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams), C.POINTER(ClEstimator),
                                                            vp, vp, vp, ll] + [vp] * 11
        L.fsaempc_cl_cone_sense_batch_device.argtypes = [C.c_int, C.POINTER(ClConeSensor), ll] + [vp] * 7
        L.fsaempc_cl_estimate_cones_batch_device.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams), C.POINTER(ClEstimator),
                                                             vp, vp, vp, ll] + [vp] * 10 + [C.POINTER(ConeMaps), C.c_int, C.POINTER(C.c_double)] + [vp] * 7
        L.fsaempc_sqp_batch_device_m.argtypes = [C.POINTER(LtvDesc), C.POINTER(Spline), C.POINTER(LtvParams)] + [vp] * 4 + \
            [C.POINTER(QpOpts), C.POINTER(SqpOpts)] + [vp] * 6 + [C.POINTER(SqpAux), vp, ll, vp]
        L.fsaempc_cl_nmpc_shift_batch_device.argtypes = [C.c_int, C.c_int, C.c_int] + [vp] * 5
        L.fsaempc_cl_nmpc_accept_batch_device.argtypes = [C.c_int, C.c_int, C.c_int] + [vp] * 10
        L.fsaempc_debug_set_dump.argtypes = [vp, C.c_int]
        L.fsaempc_track_last_error.restype = C.c_char_p
        L.fsaempc_track_from_csv.argtypes = [C.c_char_p, C.c_int, C.POINTER(TrackTable)]
        L.fsaempc_track_from_points.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(TrackTable)]
        L.fsaempc_track_free.argtypes = [C.POINTER(TrackTable)]
        L.fsaempc_track_save.argtypes = [C.POINTER(TrackTable), C.c_char_p]
        L.fsaempc_track_load.argtypes = [C.c_char_p, C.POINTER(TrackTable)]
        _LIB = L
    return _LIB


def check(rc, what):
    if rc != 0:
        raise FsaempcError("%s failed (%d): %s" % (what, rc, lib().fsaempc_last_error().decode()))


def default_params(model):
    """The FSAEMPC_NPAR defaults of `model` (fsaempc_ltv_default_params; a host function: no GPU needed) as a (32,) numpy array."""
    import numpy as np
    out = np.zeros(NPAR, dtype=np.float64)
    check(lib().fsaempc_ltv_default_params(int(model), out.ctypes.data_as(C.POINTER(C.c_double))), "fsaempc_ltv_default_params")
    return out


class ParamBlock:
    """Device copy of a parameter block, (32,) shared by the batch or (batch, 32) per instance (numpy or a device tensor), and the
    fsaempc_ltv_params that points at it."""

    def __init__(self, params, batch, device):
        import numpy as np
        import torch
        t = params if isinstance(params, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(params, dtype=np.float64)))
        if tuple(t.shape) not in ((NPAR,), (batch, NPAR)):
            raise ValueError("params must be (%d,) or (batch = %d, %d), got %s" % (NPAR, batch, NPAR, tuple(t.shape)))
        self.tensor = t.to(device=device, dtype=torch.float64).contiguous()
        self.per_instance = 1 if t.dim() == 2 else 0
        self.c = LtvParams(C.c_void_p(self.tensor.data_ptr()), self.per_instance)

    def ref(self):
        return C.byref(self.c)


def sqp_default_opts(**kw):
    o = SqpOpts()
    lib().fsaempc_sqp_default_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("unknown SQP option %r" % k)
        setattr(o, k, v)
    return o


def default_opts(**kw):
    o = QpOpts()
    lib().fsaempc_qp_default_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o
