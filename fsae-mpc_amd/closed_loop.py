"""Host-side mirror of the reference's closed loop (main.m:91-179) for a batch of independent cars: frame transform +
reference -> LTV-MPC step -> actuator/plant sub-steps, every stage a device kernel behind the C ABI."""
import ctypes as C

import numpy as np

from ._lib import (CL_MAX_DELAY, CONE_OBS_MAX, CONES_MAX, LAP_STATE_INDEX, METRIC_INDEX, NLAPSTATE, NMETRIC, NREPORT, REPORT_INDEX, ClConeSensor, ClEstimator, ClLatency, ClSensors, ConeMaps, ParamBlock, Spline, check,
                   check_blocking, check_laps, lib)
from .ltvmpc import LtvBatch, dims
from .corridor import check_corridor
from .plan import Plan


class LapReport:
    """The per-car records of a closed-loop run (include/fsaempc.h FSAEMPC_M_*; main.m:196-228 per car) on the host.  Every slot is an
    attribute by its lower-case name (steps, status, n_viol_int, ...), one entry per car; lap_time = steps * dt (a lap only for
    the cars with status == 1).  summary() is the batch summary of fsaempc_cl_report as a dict (lower-case FSAEMPC_R_* names).

    Multi-lap runs (ClosedLoop(laps > 1)) hand in what the lap gate kept: lap_times (B, laps) with NaN for a lap not
    completed, lap_state (B, 4) and lap_records (B, laps, 16).  Then `metrics` -- and with it every slot attribute and summary() -- is the
    record of the lap each car is driving (or of its last lap, once it finished); laps_done counts the completed laps; lap_records holds
    rows 0 .. laps_done - 1 from the gate and the car's current or latched record in row laps_done (row laps - 1 for a car that finished);
    lap_time is the sum of the completed laps' times.  Without them (laps == 1) the same attributes describe the single lap: laps_done is
    1 for a finished car, lap_times (B, 1) is its lap_time (NaN for the others), lap_records (B, 1, 16) is metrics.  lap_summary() is the
    (laps, 4) table of fsaempc_cl_lap_summary: per lap the cars that completed it, then mean, min and max of its time."""

    def __init__(self, metrics, dt, lap_times=None, lap_state=None, lap_records=None):
        self.metrics = np.ascontiguousarray(np.asarray(metrics, dtype=np.float64).reshape(-1, NMETRIC))
        self.dt = float(dt)
        for name, i in METRIC_INDEX.items():
            setattr(self, name.lower(), self.metrics[:, i])
        B = self.metrics.shape[0]
        if lap_times is None:
            self.laps = 1
            self.lap_time = self.steps * self.dt
            self.laps_done = (self.status == 1.0).astype(np.int64)
            self.lap_times = np.where(self.status == 1.0, self.lap_time, np.nan).reshape(B, 1)
            self.lap_records = self.metrics.reshape(B, 1, NMETRIC)
            return
        self.lap_times = np.ascontiguousarray(np.asarray(lap_times, dtype=np.float64).reshape(B, -1))
        self.laps = self.lap_times.shape[1]
        self.laps_done = np.asarray(lap_state, dtype=np.float64).reshape(B, NLAPSTATE)[:, LAP_STATE_INDEX["DONE"]].astype(np.int64)
        self.lap_records = np.array(np.asarray(lap_records, dtype=np.float64).reshape(B, self.laps, NMETRIC))
        self.lap_records[np.arange(B), np.minimum(self.laps_done, self.laps - 1)] = self.metrics
        self.lap_time = np.where(np.isnan(self.lap_times), 0.0, self.lap_times).sum(axis=1)

    def lap_summary(self):
        out = np.zeros((self.laps, 4))
        check(lib().fsaempc_cl_lap_summary(C.c_void_p(self.lap_times.ctypes.data) if self.lap_times.size else None, self.lap_times.shape[0], self.laps,
                                           C.c_void_p(out.ctypes.data)), "fsaempc_cl_lap_summary")
        return out

    def summary(self):
        out = np.zeros(NREPORT)
        check(lib().fsaempc_cl_report(C.c_void_p(self.metrics.ctypes.data), self.metrics.shape[0], C.c_double(self.dt), C.c_void_p(out.ctypes.data)),
              "fsaempc_cl_report")
        return {name.lower(): float(out[i]) for name, i in REPORT_INDEX.items()}


class Latency:
    """The imperfections of a closed loop, validated here without a library call.  delay: whole MPC periods (0 ..
    CL_MAX_DELAY) between the state a plan is solved from and the period in which the plant follows it.  compensate: solve from the
    observed state predicted over those periods (needs delay >= 1).  sigma: None, or the standard deviations of the state-estimate
    noise in the model's state layout, (nx,) for the batch or (B, nx) per car, finite and >= 0 (a zero leaves the component exact).
    seed, id0: the noise of car b depends on (seed, id0 + b, period, component) only -- id0 is a shard's first global id."""

    def __init__(self, delay=0, compensate=False, sigma=None, seed=0, id0=0):
        def integer(v, name):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s must be an integer" % name)
            return int(v)
        self.delay = integer(delay, "delay")
        if not 0 <= self.delay <= CL_MAX_DELAY:
            raise ValueError("delay must be 0 .. %d" % CL_MAX_DELAY)
        if not isinstance(compensate, (bool, np.bool_)) and compensate not in (0, 1):
            raise ValueError("compensate must be True or False")
        self.compensate = bool(compensate)
        if self.compensate and self.delay < 1:
            raise ValueError("compensate needs delay >= 1")
        self.seed = integer(seed, "seed")
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must be in [0, 2^64)")
        self.id0 = integer(id0, "id0")
        if not 0 <= self.id0 < 2 ** 63:
            raise ValueError("id0 must be >= 0 (and below 2^63)")
        if sigma is not None:
            try:
                sigma = np.array(sigma, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("sigma must be an array of numbers")
            if sigma.ndim not in (1, 2) or sigma.shape[-1] not in (5, 7):
                raise ValueError("sigma must be (nx,) or (B, nx), got %s" % (sigma.shape,))
            if not np.isfinite(sigma).all() or (sigma < 0).any():
                raise ValueError("sigma must be finite and >= 0")
        self.sigma = sigma

    @property
    def engaged(self):
        return self.delay > 0 or self.sigma is not None

    def check_batch(self, nx, B):
        """The shape of sigma against the model and the batch of the loop that takes it."""
        if self.sigma is not None and self.sigma.shape not in ((nx,), (B, nx)):
            raise ValueError("sigma must be (nx = %d,) or (B = %d, %d), got %s" % (nx, B, nx, self.sigma.shape))


def check_latency(latency, nx, B):
    """Validates ClosedLoop's latency argument (no library call): None or a Latency whose sigma fits (nx,) or (B, nx)."""
    if latency is None:
        return None
    if not isinstance(latency, Latency):
        raise ValueError("latency must be None or a Latency")
    latency.check_batch(nx, B)
    return latency


class Estimator:
    """The state estimator of a closed loop: one extended Kalman filter per car between the observation and the MPC
    step, validated here without a library call.  All variances are in the model's state layout.  q: process variances per MPC
    period, (nx,) for the batch or (B, nx) per car, finite and >= 0.  r: measurement variances, (nx,) or (B, nx), each finite and
    >= 0 or +inf ("this component is not measured"); None = the squares of the loop's Latency.sigma.  p0: initial variances, (nx,),
    finite and > 0; None = r where r is finite and > 0, else 1.0 (needs an r for the batch).  In a loop with CartesianSensors
     r is read in the sensor layout, [X, Y, psi, ...], and None = the squares of the sensors' sigma; q and p0 stay in
    the state layout (so a default p0 takes the sensor variances of (X, Y, psi) for (s, n, mu): the same units)."""

    def __init__(self, q, r=None, p0=None):
        def array(v, name):
            try:
                a = np.array(v, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("%s must be an array of numbers" % name)
            return a
        q = array(q, "q")
        if q.ndim not in (1, 2) or q.shape[-1] not in (5, 7):
            raise ValueError("q must be (nx,) or (B, nx), got %s" % (q.shape,))
        if not np.isfinite(q).all() or (q < 0).any():
            raise ValueError("q must be finite and >= 0")
        if r is not None:
            r = array(r, "r")
            if r.ndim not in (1, 2) or r.shape[-1] != q.shape[-1]:
                raise ValueError("r must be (nx,) or (B, nx) with the nx of q, got %s" % (r.shape,))
            if np.isnan(r).any() or (r < 0).any():
                raise ValueError("r must be >= 0 (+inf: the component is not measured)")
        if p0 is not None:
            p0 = array(p0, "p0")
            if p0.shape != (q.shape[-1],):
                raise ValueError("p0 must be (nx,), got %s" % (p0.shape,))
            if not np.isfinite(p0).all() or (p0 <= 0).any():
                raise ValueError("p0 must be finite and > 0")
        elif r is not None and r.ndim != 1:
            raise ValueError("p0 must be given with a per-car r")
        self.q, self.r, self.p0 = q, r, p0

    def resolve(self, latency, nx, B, laps=1, sensors=None):
        """(q, r, p0) for a loop of B cars with nx states: shapes checked, r and p0 filled in from their defaults."""
        if self.q.shape not in ((nx,), (B, nx)):
            raise ValueError("q must be (nx = %d,) or (B = %d, %d), got %s" % (nx, B, nx, self.q.shape))
        r = self.r
        if r is None and sensors is not None:
            r = sensors.sigma ** 2
        if r is None:
            if latency is None or latency.sigma is None:
                raise ValueError("Estimator(r=None) takes the variances of a Latency with sigma")
            r = latency.sigma ** 2
        if r.shape not in ((nx,), (B, nx)):
            raise ValueError("r must be (nx = %d,) or (B = %d, %d), got %s" % (nx, B, nx, r.shape))
        p0 = self.p0
        if p0 is None:
            if r.ndim != 1:
                raise ValueError("p0 must be given with a per-car r")
            p0 = np.where(np.isfinite(r) & (r > 0), r, 1.0)
        if sensors is None and laps > 1 and np.isinf(r[..., 0]).any():   # (with sensors the re-basing reads the projection)
            raise ValueError("laps > 1 needs a measured arc length (r[0] finite): the estimate is re-based on it at the line")
        return self.q, r, p0


def check_estimator(estimator, latency, nx, B, laps=1, sensors=None):
    """Validates ClosedLoop's estimator argument (no library call): None, or an Estimator resolved to (q, r, p0)."""
    if estimator is None:
        return None
    if not isinstance(estimator, Estimator):
        raise ValueError("estimator must be None or an Estimator")
    return estimator.resolve(latency, nx, B, laps, sensors)


class CartesianSensors:
    """The Cartesian sensor models of a closed loop, validated here without a library call.  sigma: the standard
    deviations of the measurement noise in the sensor layout -- the model's state layout with (s, n, mu) replaced by (X, Y, psi):
    kinematic [X, Y, psi, v, delta], dynamic [X, Y, psi, x_d, y_d, theta_d, delta] -- (nx,) for the batch or (B, nx) per car, finite
    and >= 0 (a zero leaves the component exact).  seed, id0: the noise of car b depends on (seed, id0 + b, period, component) only,
    as Latency's."""

    def __init__(self, sigma, seed=0, id0=0):
        def integer(v, name):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s must be an integer" % name)
            return int(v)
        self.seed = integer(seed, "seed")
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must be in [0, 2^64)")
        self.id0 = integer(id0, "id0")
        if not 0 <= self.id0 < 2 ** 63:
            raise ValueError("id0 must be >= 0 (and below 2^63)")
        try:
            sigma = np.array(sigma, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("sigma must be an array of numbers")
        if sigma.ndim not in (1, 2) or sigma.shape[-1] not in (5, 7):
            raise ValueError("sigma must be (nx,) or (B, nx), got %s" % (sigma.shape,))
        if not np.isfinite(sigma).all() or (sigma < 0).any():
            raise ValueError("sigma must be finite and >= 0")
        self.sigma = sigma

    def check_batch(self, nx, B):
        """The shape of sigma against the model and the batch of the loop that takes it."""
        if self.sigma.shape not in ((nx,), (B, nx)):
            raise ValueError("sigma must be (nx = %d,) or (B = %d, %d), got %s" % (nx, B, nx, self.sigma.shape))


def check_sensors(sensors, latency, nx, B):
    """Validates ClosedLoop's sensors argument (no library call): None, or a CartesianSensors whose sigma fits (nx,) or (B, nx), next
    to a latency that adds no noise of its own."""
    if sensors is None:
        return None
    if not isinstance(sensors, CartesianSensors):
        raise ValueError("sensors must be None or a CartesianSensors")
    sensors.check_batch(nx, B)
    if latency is not None and latency.sigma is not None:
        raise ValueError("sensors and Latency(sigma=...) are two noise sources: with sensors the latency carries the delay only")
    return sensors


class ConeSensor:
    """The cone sensor of a closed loop and the cone rows of its filter, validated here without a library call.  left,
    right: (K_l, 2) / (K_r, 2) positions of the cones that stand on the track (the truth the sensor reads), at most CONES_MAX per side.
    r_min, r_max (m), fov (rad, the whole opening angle, centred on the heading): the view.  sigma = (range m, bearing rad): the noise,
    finite and >= 0.  p_detect: the probability that a cone in view is detected.  k_max: observations per car and period, the nearest
    ones, 1 .. CONE_OBS_MAX.  seed, id0: the draws of car b and cone g depend on (seed, id0 + b, period, g) only.  map_left, map_right:
    the map the filter reads, None = the truth; (K, 2) for the batch or (B, K, 2) one per car (cone_draws: a Monte-Carlo over the
    mapping error), with the truth's counts.  r = (range, bearing) variances of the filter's cone rows, each >= 0 or +inf ("this channel is
    off": r = (inf, v) is a bearing-only camera); None = sigma^2."""

    def __init__(self, left, right, r_max=15.0, r_min=0.5, fov=2 * np.pi / 3, sigma=(0.05, 0.01), p_detect=1.0, k_max=16, seed=0, id0=0,
                 map_left=None, map_right=None, r=None):
        def integer(v, name):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s must be an integer" % name)
            return int(v)

        def number(v, name):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError("%s must be a number" % name)
            return float(v)

        def side(v, name, ndims):
            try:
                a = np.array(v, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("%s must be an array of numbers" % name)
            if a.ndim == ndims[0] and a.size == 0:
                a = a.reshape((0, 2))
            if a.ndim not in ndims or a.shape[-1] != 2:
                raise ValueError("%s must be (K, 2)%s, got %s" % (name, " or (B, K, 2)" if len(ndims) > 1 else "", a.shape))
            if a.shape[-2] > CONES_MAX:
                raise ValueError("%s: at most %d cones per side" % (name, CONES_MAX))
            return np.ascontiguousarray(a)
        self.left, self.right = side(left, "left", (2,)), side(right, "right", (2,))
        if self.left.shape[0] + self.right.shape[0] == 0:
            raise ValueError("a cone map with no cones")
        self.r_min, self.r_max, self.fov = number(r_min, "r_min"), number(r_max, "r_max"), number(fov, "fov")
        if not (self.r_max < float("inf")) or not (self.r_min > 0) or not (self.r_min < self.r_max):
            raise ValueError("r_min must be > 0 and below a finite r_max")
        if not (0 < self.fov <= 2 * np.pi):
            raise ValueError("fov must be in (0, 2 pi]")
        try:
            sg = np.array(sigma, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("sigma must be two numbers")
        if sg.shape != (2,) or not np.isfinite(sg).all() or (sg < 0).any():
            raise ValueError("sigma must be (range, bearing), finite and >= 0")
        self.sigma = sg
        self.p_detect = number(p_detect, "p_detect")
        if not (0 <= self.p_detect <= 1):
            raise ValueError("p_detect must be in [0, 1]")
        self.k_max = integer(k_max, "k_max")
        if not 1 <= self.k_max <= CONE_OBS_MAX:
            raise ValueError("k_max must be 1 .. %d" % CONE_OBS_MAX)
        self.seed = integer(seed, "seed")
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must be in [0, 2^64)")
        self.id0 = integer(id0, "id0")
        if not 0 <= self.id0 < 2 ** 63:
            raise ValueError("id0 must be >= 0 (and below 2^63)")
        if (map_left is None) != (map_right is None):
            raise ValueError("map_left and map_right are given together")
        if map_left is None:
            self.map_left, self.map_right = self.left, self.right
        else:
            self.map_left, self.map_right = side(map_left, "map_left", (2, 3)), side(map_right, "map_right", (2, 3))
            if self.map_left.ndim != self.map_right.ndim or (self.map_left.ndim == 3 and self.map_left.shape[0] != self.map_right.shape[0]):
                raise ValueError("map_left and map_right are both shared or both per car")
            if self.map_left.shape[-2] != self.left.shape[0] or self.map_right.shape[-2] != self.right.shape[0]:
                raise ValueError("the map must have the truth's counts (%d left, %d right), got %d and %d"
                                 % (self.left.shape[0], self.right.shape[0], self.map_left.shape[-2], self.map_right.shape[-2]))
        if r is None:
            self.r = sg ** 2
        else:
            try:
                self.r = np.array(r, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("r must be two numbers")
            if self.r.shape != (2,) or np.isnan(self.r).any() or (self.r < 0).any():
                raise ValueError("r must be (range, bearing), each >= 0 (+inf: the channel is off)")

    def check_batch(self, B):
        """A per-car map against the batch of the loop that takes it."""
        if self.map_left.ndim == 3 and self.map_left.shape[0] != B:
            raise ValueError("a per-car map must be (B = %d, K, 2), got %s" % (B, self.map_left.shape))


def check_cones(cones, sensors, estimator, B):
    """Validates ClosedLoop's cones argument (no library call): None, or a ConeSensor next to sensors and an estimator."""
    if cones is None:
        return None
    if not isinstance(cones, ConeSensor):
        raise ValueError("cones must be None or a ConeSensor")
    if sensors is None:
        raise ValueError("cones needs sensors=CartesianSensors(...): the filter with the cone rows reads the Cartesian measurement")
    if estimator is None:
        raise ValueError("cones needs estimator=Estimator(...): the cone observations are rows of the filter")
    cones.check_batch(B)
    return cones


class Nmpc:
    """The batched SQP of the nonlinear MPC step as the controller of a closed loop (main.m:118-160, MODE =
    "MS-NMPC"), validated here without a library call.  sweeps: the sweep cap of a period (max_sweeps; 1 is a real-time iteration).
    skip_finished: cars that no longer drive are masked out of the SQP's sub-batch.  sqp_opts: the other fields of fsaempc_sqp_opts
    (trials, tol_step, tol_feas, armijo, rho0, warm_start)."""

    OPTIONS = ("trials", "tol_step", "tol_feas", "armijo", "rho0", "warm_start")

    def __init__(self, sweeps=1, skip_finished=True, **sqp_opts):
        def integer(v, name):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s must be an integer" % name)
            return int(v)
        self.sweeps = integer(sweeps, "sweeps")
        if self.sweeps < 1:
            raise ValueError("sweeps must be >= 1")
        if not isinstance(skip_finished, (bool, np.bool_)):
            raise ValueError("skip_finished must be True or False")
        self.skip_finished = bool(skip_finished)
        self.sqp_opts = {}
        for k, v in sqp_opts.items():
            if k == "max_sweeps":
                raise ValueError("the sweep cap is Nmpc(sweeps=...)")
            if k not in self.OPTIONS:
                raise ValueError("unknown SQP option %r (known: %s)" % (k, ", ".join(self.OPTIONS)))
            if k == "trials":
                v = integer(v, k)
                if not 1 <= v <= 64:
                    raise ValueError("trials must be 1 .. 64")
            elif k == "warm_start":
                if not isinstance(v, (bool, np.bool_)) and not (isinstance(v, (int, np.integer)) and v in (0, 1)):
                    raise ValueError("warm_start must be 0 or 1")
                v = int(v)
            else:
                if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 <= float(v) < float("inf"):
                    raise ValueError("%s must be a finite number >= 0" % k)
                v = float(v)
            self.sqp_opts[k] = v


def check_controller(controller, corridor, blocking, N, warm_start):
    """Validates ClosedLoop's controller argument against the arguments the SQP has no form for (no library call)."""
    if controller is None:
        return None
    if not isinstance(controller, Nmpc):
        raise ValueError("controller must be None (the LTV-MPC step) or an Nmpc")
    if corridor is not None:
        raise NotImplementedError("SqpBatch (the exact build of the NLP, nlp_build_qp) is not available with a corridor; "
                                  "LtvBatch(..., corridor=...).sqp re-linearises a batch inside a corridor")
    if blocking is not None and len(check_blocking(blocking, N)) != N:
        raise NotImplementedError("SqpBatch (the exact build of the NLP, nlp_build_qp) is not available with move blocking; "
                                  "LtvBatch(..., blocking=...).sqp re-linearises a blocked batch")
    if warm_start:
        raise ValueError("warm_start is the initial point of the LTV step's QP (fsaempc_qp_aux.x_init); the SQP has its own option, Nmpc(warm_start=...)")
    return controller


def nmpc_shift(u_keep, finished, shift, u_init, skip, stream=None):
    """fsaempc_cl_nmpc_shift_batch_device on device tensors: u_init (B, N, 2) = u_keep shifted by one stage (shift = 1) or copied
    (shift = 0), skip (B,) int32 = finished != 0 (finished may be None: all zero)."""
    import torch
    B, N = u_keep.shape[0], u_keep.shape[1]
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(u_keep.device).cuda_stream)
    check(lib().fsaempc_cl_nmpc_shift_batch_device(N, B, int(shift), P(u_keep), P(finished), P(u_init), P(skip), st), "fsaempc_cl_nmpc_shift_batch_device")


def nmpc_accept(model, N, x_new, u_new, status, qp_iter, skip, x_keep, u_keep, exitflag, iter, stream=None):
    """fsaempc_cl_nmpc_accept_batch_device on device tensors (qp_iter and skip may be None)."""
    import torch
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(x_keep.device).cuda_stream)
    check(lib().fsaempc_cl_nmpc_accept_batch_device(int(model), int(N), status.shape[0], P(x_new), P(u_new), P(status), P(qp_iter), P(skip), P(x_keep),
                                                    P(u_keep), P(exitflag), P(iter), st), "fsaempc_cl_nmpc_accept_batch_device")


def cl_noise(nx, B, seed, id0, step, device="cuda:0"):
    """The (B, nx) standard normals the observation of period `step` draws for cars id0 .. id0 + B - 1
    (fsaempc_cl_noise_batch_device), a device tensor."""
    import torch
    z = torch.empty((int(B), int(nx)), dtype=torch.float64, device=device)
    check(lib().fsaempc_cl_noise_batch_device(int(nx), int(B), C.c_ulonglong(int(seed)), C.c_longlong(int(id0)), C.c_longlong(int(step)),
                                              C.c_void_p(z.data_ptr()), C.c_void_p(torch.cuda.current_stream(z.device).cuda_stream)),
          "fsaempc_cl_noise_batch_device")
    return z


class ClosedLoop:
    """B cars on one track.  cart0: (B, 7) Cartesian states [x, y, theta, x_d, y_d, theta_d, delta] (main.m:63 starts
    from zeros(7,1)).  step() advances every car by one MPC period dt, all on the device and without reading anything
    back; like the reference (main.m:122-126, 163-175) a car keeps driving after an abnormal solver exit -- on its last good
    plan -- and the exit flags are only tallied.  Cars that completed the lap (s >= L) or left the track keep their state."""

    def __init__(self, model, N, dt, track, cart0, target_vel=20.0, device="cuda:0", options=None, integrator=-1, warm_start=False, launch_hint=True,
                 params=None, plant_params=None, blocking=None, reference=None, metrics=False, slack_tol=1e-6, corridor=None, laps=1,
                 latency=None, estimator=None, controller=None, sensors=None, cones=None):
        """params: parameter block(s) of the controller ((32,) or (B, 32), as for LtvBatch); plant_params: the cars' own block(s),
        None = the same as params (both None: the reference's constants compiled into the kernels).  blocking: block lengths of the
        controller's held inputs (LtvBatch); the plan the loop carries stays the expanded one, (B, N, 2).  reference: None = the live
        generator of main.m:107-114 (a ramp to target_vel); a Plan = main.m:115, the cars track it (shared, or one table per car;
        target_vel is then unused).  metrics: keep the lap report's per-car records (self.metrics, (B, 16) on the device; one more
        kernel per step, on the same stream; limits and ellipse axes are those of params) -- report() reads them back.  slack_tol: a slack
        counts as in use above it (the reference tests == 0; 1e-6 is this build's solve tolerance).  corridor: None or a Corridor (shared,
        or one per car): the controller's track rows and, with metrics, the report's track violation are taken against it
        (DESIGN.md 6l).  laps: 1 = the run of a car ends the first time s >= L (main.m:102-104); K > 1 = the lap gate (lap_gate(), one more
        kernel per step between pre() and the MPC step) carries it over the line K - 1 times: self.lap_times (B, K) holds the laps' times
        to a fraction of dt (NaN: not completed), self.lap_state (B, 4) the gate's state (LAP_STATE_INDEX), and with metrics
        self.lap_records (B, K, 16) the closed laps' records while self.metrics is the record of the lap being driven.
        latency: None or a Latency.  None, or one with delay 0 and no sigma, is the ideal loop: step() launches what it
        launches without the argument.  Otherwise step() observes the state after pre() and the lap gate (self.x0_obs = x0 + noise),
        predicts it over the delay if asked to (self.x0_mpc), regenerates x_ref from x0_mpc, solves from x0_mpc, and the plant follows
        the plan accepted `delay` periods ago (self.plant_plan, a view of self.x_hist (delay + 1, B, N, nx); self.u_hist likewise).
        self.x0 stays the true state (the gate and the metrics read it); self.x_opt / self.u_opt stay the newest plan.
        estimator: None or an Estimator.  None launches what the loop launches without the argument.  Otherwise step()
        observes with the noise alone (self.x0_obs; without a latency the measurement is x0), filters it (self.x0_est, with the carried
        self.est_x, self.est_P (B, nx, nx), self.est_count (B, 2); self.est_innov, self.est_nis and self.est_resets of the period), predicts
        x0_est over the delay if the latency compensates (self.x0_mpc; otherwise self.x0_mpc is self.x0_est), regenerates x_ref from the
        state the solve reads and solves from it.  The filter's input is the first input of the plan the plant followed in the period
        just past.
        controller: None = the LTV-MPC step (main.m MODE = "LTV-MPC"): step() launches what it launches without the argument and
        nothing more is allocated.  An Nmpc = the batched SQP of the nonlinear problem (MODE = "MS-NMPC").  step() then
        runs pre, lap gate, observation / estimator as before, shifts the kept plan by one stage into self.u_init (unshifted in the
        first period) and masks the cars that no longer drive (self.nmpc_skip), solves with self.sqp (a SqpBatch on the same track,
        params, integrator and options) from the state the LTV step would have read, and takes the result over
        (fsaempc_cl_nmpc_accept_batch_device: every finite result, whatever the status); history slots, plant and metrics follow
        as before.  self.nmpc_status is the SQP's verbatim status of the last period; the returned exitflag is 0 for status 0 and 1
        and the status otherwise.  self.mpc stays: its descriptor, spline and params serve the observer, the estimator and the
        metrics.  The SQP call blocks the host once per sweep (it reads the number of instances still running), so in this mode step()
        is no longer free of read-backs.  Not available with corridor=, a non-trivial blocking= (NotImplementedError) or
        warm_start=True (ValueError: that flag is the QP's x_init; Nmpc(warm_start=...) is the SQP's own).
        sensors: None or a CartesianSensors.  None launches what the loop launches without the argument.  Otherwise
        step() measures the car in the Cartesian frame after pre() and the lap gate (self.y_meas, sensor layout) and projects the
        measurement onto the track (self.x_proj; self.proj_lost counts the projections that lost the track and fell back to x0).
        With an estimator the filter reads y_meas through h(x) (fsaempc_cl_estimate_cart_batch_device; Estimator.r in the sensor
        layout, None = sigma^2; first prior, re-initialisation and re-basing from x_proj, so laps > 1 needs no measured arc length);
        without one the loop drives on x_proj.  The latency's prediction then runs on that state if it compensates, x_ref is
        regenerated and the controller solves from it.  self.x0 stays the true state (the gate and the metrics read it).  Not
        together with a Latency that has a sigma (ValueError: two noise sources).
        cones: None or a ConeSensor, next to sensors and an estimator (ValueError without either).  None launches what
        the loop launches without the argument.  Otherwise step() runs pre, lap gate, sense, the cone sensor
        (fsaempc_cl_cone_sense_batch_device on the true pose: self.cone_n, self.cone_seen (B,), self.cone_id (B, k_max), self.cone_z
        (B, k_max, 2)) and the filter with the cone rows in the place of the Cartesian filter
        (fsaempc_cl_estimate_cones_batch_device: self.cone_innov (B, k_max, 2), self.est_rows (B,) the rows applied, next to the
        estimator's attributes), then whatever followed before.  A GPS outage is Estimator(r=[inf, inf, inf, ...]): the pose rows
        are off and the cones carry the pose; the first prior, the re-initialisation state and the re-basing still read x_proj, the
        projection of the (noisy) pose measurement."""
        self.controller = check_controller(controller, corridor, blocking, N, warm_start)   # (before the library is touched)
        if not (float(slack_tol) >= 0):
            raise ValueError("slack_tol must be >= 0")
        self.laps = check_laps(laps)   # (before the library is touched)
        if blocking is not None:
            check_blocking(blocking, N)   # (before the library is touched)
        if reference is not None:
            if not isinstance(reference, Plan):
                raise ValueError("reference must be None or a Plan")
            reference.check_batch(np.asarray(cart0).size // 7)
            reference.check_device(device)
        self.reference = reference
        check_corridor(corridor, np.asarray(cart0).size // 7, device)   # (before the library is touched)
        self.latency = check_latency(latency, 5 if model == 0 else 7, np.asarray(cart0).size // 7)   # (likewise)
        self.sensors = check_sensors(sensors, self.latency, 5 if model == 0 else 7, np.asarray(cart0).size // 7)   # (likewise)
        self._est_arrays = check_estimator(estimator, latency, 5 if model == 0 else 7, np.asarray(cart0).size // 7, self.laps, self.sensors)   # (likewise)
        self.cones = check_cones(cones, self.sensors, estimator, np.asarray(cart0).size // 7)   # (likewise)
        self.estimator = estimator
        if self.latency is not None and not self.latency.engaged:
            self.latency = None
        import torch
        self.torch = torch
        self.device = torch.device(device)
        self.model, self.N, self.dt, self.target_vel = model, N, float(dt), float(target_vel)
        self.nx = dims(model, N)[0]
        cart0 = np.ascontiguousarray(np.asarray(cart0, dtype=np.float64).reshape(-1, 7))
        self.B = cart0.shape[0]
        self.track = track
        self.mpc = LtvBatch(model, N, dt, track, self.B, device=device, options=options, integrator=integrator, params=params,
                            blocking=blocking, corridor=corridor)
        self.corridor = self.mpc.corridor
        if plant_params is None:
            plant_params = params
        self.plant_params = ParamBlock(plant_params, self.B, self.device) if plant_params is not None else None
        self.cart = torch.from_numpy(cart0).to(self.device)
        self.pid = torch.zeros((self.B, 4), dtype=torch.float64, device=self.device)
        self.finished = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        # MPC initial guess of main.m:47-55: quadratic arc length, linear velocity, constant acceleration 10
        k = np.arange(1, N + 1, dtype=np.float64) * self.dt
        x_opt = np.zeros((self.B, N, self.nx)); u_opt = np.zeros((self.B, N, 2))
        x_opt[:, :, 0] = 10 * k ** 2 / 2
        x_opt[:, :, 3] = 10 * k
        u_opt[:, :, 0] = 10
        self.x_opt = torch.from_numpy(x_opt).to(self.device)
        self.u_opt = torch.from_numpy(u_opt).to(self.device)
        self.x0 = torch.empty((self.B, self.nx), dtype=torch.float64, device=self.device)
        self.x_ref = torch.empty((self.B, N, self.nx), dtype=torch.float64, device=self.device)
        self.u_last = torch.zeros((self.B, 2), dtype=torch.float64, device=self.device)
        self.steps = 0
        self.slack_tol = float(slack_tol)
        self.x0_obs = self.x0_mpc = self.x_hist = self.u_hist = None
        self.plant_plan = self.x_opt
        if self.latency is not None:
            lat = self.latency
            self.x0_obs = torch.empty_like(self.x0)
            self.x0_mpc = torch.empty_like(self.x0)
            self._s0_mpc = torch.empty(self.B, dtype=torch.float64, device=self.device)
            self._sigma = torch.from_numpy(lat.sigma).to(self.device).contiguous() if lat.sigma is not None else None
            self._lat = ClLatency(lat.delay, int(lat.compensate), C.c_void_p(self._sigma.data_ptr()) if self._sigma is not None else None,
                                  1 if self._sigma is not None and self._sigma.dim() == 2 else 0, lat.seed, lat.id0)
            if lat.delay > 0:   # the history is filled from x_opt / u_opt at the first step(): callers edit the initial guess before it
                self.x_hist = torch.empty((lat.delay + 1, self.B, N, self.nx), dtype=torch.float64, device=self.device)
                self.u_hist = torch.empty((lat.delay + 1, self.B, N, 2), dtype=torch.float64, device=self.device)
        self.x0_est = self.est_x = self.est_P = self.est_count = self.est_innov = self.est_nis = self.est_x_start = None
        if self.estimator is not None:
            q, r, p0 = self._est_arrays
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=self.device)
            self._est_q, self._est_r, self._est_p0 = dev(q), dev(r), dev(p0)
            self._est = ClEstimator(C.c_void_p(self._est_q.data_ptr()), 1 if q.ndim == 2 else 0, C.c_void_p(self._est_r.data_ptr()), 1 if r.ndim == 2 else 0,
                                    C.c_void_p(self._est_p0.data_ptr()), self.track.L if self.laps > 1 else 0.0)
            self.x0_est, self.est_x, self.est_innov, self.est_x_start = f64(self.B, self.nx), f64(self.B, self.nx), f64(self.B, self.nx), f64(self.B, self.nx)
            self.est_P, self.est_nis = f64(self.B, self.nx, self.nx), f64(self.B)
            self.est_count = torch.zeros((self.B, 2), dtype=torch.int32, device=self.device)
            if self.latency is None:
                self._s0_mpc = torch.empty(self.B, dtype=torch.float64, device=self.device)
                self.x0_mpc = self.x0_est
            else:   # the two existing observe calls of an engaged period: noise alone (delay 0), then the predictor alone (no sigma)
                lat = self.latency
                self._obs_scratch = torch.empty_like(self.x0)
                self._lat_noise = ClLatency(0, 0, self._lat.sigma, self._lat.sigma_per_instance, lat.seed, lat.id0)
                self._lat_pred = ClLatency(lat.delay, int(lat.compensate), None, 0, lat.seed, lat.id0)
                if not lat.compensate:
                    self.x0_mpc = self.x0_est
        self.y_meas = self.x_proj = self.proj_lost = None
        if self.sensors is not None:
            self._sens_sigma = torch.from_numpy(np.ascontiguousarray(self.sensors.sigma)).to(self.device)
            self._sens = ClSensors(C.c_void_p(self._sens_sigma.data_ptr()), 1 if self._sens_sigma.dim() == 2 else 0, self.sensors.seed, self.sensors.id0)
            self.y_meas = torch.zeros_like(self.x0)
            self.x_proj = torch.zeros_like(self.x0)
            self.proj_lost = torch.zeros(self.B, dtype=torch.int32, device=self.device)
            if self.estimator is None and self.latency is None:
                self._s0_mpc = torch.empty(self.B, dtype=torch.float64, device=self.device)
                self.x0_mpc = self.x_proj
        self.cone_n = self.cone_seen = self.cone_id = self.cone_z = self.cone_innov = self.est_rows = None
        if self.cones is not None:
            cs = self.cones
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
            self._cone_arrays = [dev(a) for a in (cs.left, cs.right)]
            self._cone_arrays += self._cone_arrays if cs.map_left is cs.left else [dev(a) for a in (cs.map_left, cs.map_right)]
            tl, tr_, ml, mr = self._cone_arrays
            self._cone_truth = ConeMaps(ptr(tl), ptr(tr_), cs.left.shape[0], cs.right.shape[0], 0)
            self._cone_map = ConeMaps(ptr(ml), ptr(mr), cs.left.shape[0], cs.right.shape[0], 1 if cs.map_left.ndim == 3 else 0)
            self._cone_sensor = ClConeSensor(C.pointer(self._cone_truth), cs.r_min, cs.r_max, cs.fov, float(cs.sigma[0]), float(cs.sigma[1]), cs.p_detect,
                                             cs.k_max, cs.seed, cs.id0)
            self._cone_r = (C.c_double * 2)(float(cs.r[0]), float(cs.r[1]))
            self.cone_n = torch.zeros(self.B, dtype=torch.int32, device=self.device)
            self.cone_seen = torch.zeros(self.B, dtype=torch.int32, device=self.device)
            self.cone_id = torch.full((self.B, cs.k_max), -1, dtype=torch.int32, device=self.device)
            self.cone_z = torch.zeros((self.B, cs.k_max, 2), dtype=torch.float64, device=self.device)
            self.cone_innov = torch.zeros((self.B, cs.k_max, 2), dtype=torch.float64, device=self.device)
            self.est_rows = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self.metrics = torch.zeros((self.B, NMETRIC), dtype=torch.float64, device=self.device) if metrics else None
        self.lap_state = self.lap_times = self.lap_records = None   # laps == 1: nothing is allocated unless lap_gate() is called
        if self.laps > 1:
            self._lap_alloc()
        # warm_start: every solve starts from the plan of the previous period shifted by one stage (fsaempc_qp_aux.x_init): the
        # inputs u_1..u_{N-1}, the last stage repeated, the previous slack values.  Off by default -- the reference's loop solves
        # cold (main.m:117-120 passes no initial guess) and the gain is modest (profiles/round3/warm_start_ab.json)
        self.warm_start = bool(warm_start)
        self._slack = None
        # launch_hint: the iteration count of each car's previous QP is handed to the solve as the effort estimate behind its launch
        # order (fsaempc_qp_aux.difficulty: a far better predictor than the library's cold estimate); results do not depend on it
        self.launch_hint = bool(launch_hint)
        self._last_iter = None
        self._x_init = torch.zeros((self.B, self.mpc.nV), dtype=torch.float64, device=self.device) if self.warm_start else None
        if self.warm_start and self.mpc.blocking is not None:
            self._shift_idx = torch.tensor([min(s + 1, N - 1) for s in self.mpc.blocking.start], dtype=torch.long, device=self.device)
        self.sqp = self.u_init = self.nmpc_skip = self.nmpc_status = None
        if self.controller is not None:
            from .sqp import SqpBatch
            self.sqp = SqpBatch(model, N, dt, track, self.B, device=device, options=options, integrator=integrator, params=params)
            self.u_init = torch.zeros((self.B, N, 2), dtype=torch.float64, device=self.device)
            self.nmpc_skip = torch.zeros(self.B, dtype=torch.int32, device=self.device)

    def _stream(self, stream):
        return C.c_void_p(stream if stream is not None else self.torch.cuda.current_stream(self.device).cuda_stream)

    def pre(self, stream=None):
        P = lambda t: C.c_void_p(t.data_ptr())
        s_guess = self.x_opt[:, 0, 0].contiguous()
        if self.reference is not None:
            rc = lib().fsaempc_cl_pre_plan_batch_device(self.model, self.N, C.c_double(self.dt), C.c_double(self.track.L), C.byref(self.mpc.sp),
                                                        self.reference.ref(), P(self.cart), P(s_guess), self.B, P(self.x0), P(self.x_ref),
                                                        P(self.finished), self._stream(stream))
            check(rc, "fsaempc_cl_pre_plan_batch_device")
            return
        rc = lib().fsaempc_cl_pre_batch_device(self.model, self.N, C.c_double(self.dt), C.c_double(self.target_vel), C.c_double(self.track.L),
                                               C.byref(self.mpc.sp), P(self.cart), P(s_guess), self.B, P(self.x0), P(self.x_ref),
                                               P(self.finished), self._stream(stream))
        check(rc, "fsaempc_cl_pre_batch_device")

    def _lap_alloc(self):
        torch = self.torch
        self.lap_state = torch.zeros((self.B, NLAPSTATE), dtype=torch.float64, device=self.device)
        self.lap_times = torch.full((self.B, self.laps), float("nan"), dtype=torch.float64, device=self.device)
        if self.metrics is not None:
            self.lap_records = torch.zeros((self.B, self.laps, NMETRIC), dtype=torch.float64, device=self.device)

    def lap_gate(self, stream=None):
        """The lap gate on what pre() left (fsaempc_cl_lap_gate_batch_device): step() calls it after pre() when laps > 1."""
        if self.lap_state is None:
            self._lap_alloc()
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        check(lib().fsaempc_cl_lap_gate_batch_device(self.nx, self.N, C.c_double(self.dt), C.c_double(self.track.L), self.laps, self.B, P(self.x0),
                                                     P(self.x_ref), P(self.x_opt), P(self.finished), P(self.lap_state), P(self.lap_times),
                                                     P(self.metrics) if self.lap_records is not None else None, P(self.lap_records),
                                                     self._stream(stream)), "fsaempc_cl_lap_gate_batch_device")

    def plant(self, exitflag, stream=None, plan=None):
        """plan: the (B, N, nx) plan the set points are read from; None = self.x_opt."""
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        rc = lib().fsaempc_cl_plant_batch_device_p(self.model, self.N, C.c_double(self.dt), self.B,
                                                   self.plant_params.ref() if self.plant_params is not None else None, P(self.cart), P(self.pid),
                                                   P(self.x_opt if plan is None else plan), P(self.finished), P(exitflag), P(self.u_last),
                                                   self._stream(stream))
        check(rc, "fsaempc_cl_plant_batch_device_p")

    def observe(self, stream=None):
        """Observation and prediction of this period on what pre() and the lap gate left in self.x0 (fsaempc_cl_observe_batch_device),
        then x_ref regenerated from x0_mpc by the reference the loop runs on."""
        self._fill_history()
        self._observe_call(self._lat, self.x0, self.x0_obs, self.x0_mpc, stream)
        self._reference_from(self.x0_mpc, stream)

    def _fill_history(self):
        if self.u_hist is not None and self.steps == 0:
            self.x_hist.copy_(self.x_opt.unsqueeze(0).expand_as(self.x_hist))
            self.u_hist.copy_(self.u_opt.unsqueeze(0).expand_as(self.u_hist))

    def _observe_call(self, lat, x0_true, x0_obs, x0_mpc, stream):
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        check(lib().fsaempc_cl_observe_batch_device(C.byref(self.mpc.desc), C.byref(self.mpc.sp), self.mpc.params.ref() if self.mpc.params is not None else None,
                                                    C.byref(lat), self.steps, P(x0_true), P(self.finished), P(self.u_hist), P(x0_obs),
                                                    P(x0_mpc), self._stream(stream)), "fsaempc_cl_observe_batch_device")

    def _reference_from(self, x0_mpc, stream):
        """x_ref regenerated from the state the solve reads, by the reference the loop runs on."""
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        if self.reference is not None:
            self._s0_mpc.copy_(x0_mpc[:, 0])
            check(lib().fsaempc_plan_reference_batch_device(self.model, self.reference.ref(), P(self._s0_mpc), C.c_double(self.dt), self.N, self.B,
                                                            P(self.x_ref), self._stream(stream)), "fsaempc_plan_reference_batch_device")
        else:
            check(lib().fsaempc_reference_live_batch_device(self.nx, self.N, C.c_double(self.dt), C.c_double(self.target_vel), self.B, P(x0_mpc),
                                                            P(self.x_ref), self._stream(stream)), "fsaempc_reference_live_batch_device")

    @property
    def est_resets(self):
        """Re-initialisations of every car's filter so far, (B,) int32 on the device (None without an estimator)."""
        return self.est_count[:, 1] if self.est_count is not None else None

    def prev_input(self):
        """The (B, N, 2) plan whose first input the plant followed in the period just past: slot (k - 1 - d) mod (d + 1) of the history, u_opt
        (still plan k - 1 before the solve) with d = 0."""
        if self.u_hist is None:
            return self.u_opt
        d = self.latency.delay
        return self.u_hist[(self.steps - 1 - d) % (d + 1)]

    def estimate(self, stream=None):
        """Observation, filter and prediction of this period on what pre() and the lap gate left in self.x0, then x_ref
        regenerated from the state the solve reads, which is returned."""
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._fill_history()
        z = self.x0
        if self.latency is not None:
            self._observe_call(self._lat_noise, self.x0, self.x0_obs, self._obs_scratch, stream)
            z = self.x0_obs
        if self.steps == 0:
            self.est_x_start.copy_(z)
        check(lib().fsaempc_cl_estimate_batch_device(C.byref(self.mpc.desc), C.byref(self.mpc.sp), self.mpc.params.ref() if self.mpc.params is not None else None,
                                                     C.byref(self._est), P(z), P(self.est_x_start), P(self.prev_input()), 2 * self.N, P(self.finished),
                                                     P(self.est_x), P(self.est_P), P(self.est_count), P(self.x0_est), P(self.est_innov), P(self.est_nis),
                                                     None, None, self._stream(stream)), "fsaempc_cl_estimate_batch_device")
        if self.latency is not None and self.latency.compensate:
            self._observe_call(self._lat_pred, self.x0_est, self._obs_scratch, self.x0_mpc, stream)
        self._reference_from(self.x0_mpc, stream)
        return self.x0_mpc

    def sense(self, stream=None):
        """Measurement and naive projection of this period on what pre() and the lap gate left (fsaempc_cl_sense_batch_device)."""
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        check(lib().fsaempc_cl_sense_batch_device(C.byref(self.mpc.desc), C.byref(self.mpc.sp), C.byref(self._sens), self.steps, P(self.cart), P(self.x0),
                                                  P(self.finished), P(self.y_meas), P(self.x_proj), P(self.proj_lost), self._stream(stream)),
              "fsaempc_cl_sense_batch_device")

    def cone_sense(self, stream=None):
        """The cone observations of this period from the true pose (fsaempc_cl_cone_sense_batch_device)."""
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        check(lib().fsaempc_cl_cone_sense_batch_device(self.B, C.byref(self._cone_sensor), self.steps, P(self.cart), P(self.finished), P(self.cone_n),
                                                       P(self.cone_seen), P(self.cone_id), P(self.cone_z), self._stream(stream)),
              "fsaempc_cl_cone_sense_batch_device")

    def sensed_state(self, stream=None):
        """Measurement, projection, filter (with an estimator) and prediction (with a compensating latency) of this period
        (DESIGN.md 6s), then x_ref regenerated from the state the solve reads, which is returned."""
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._fill_history()
        self.sense(stream)
        state = self.x_proj
        if self.cones is not None:
            self.cone_sense(stream)
            check(lib().fsaempc_cl_estimate_cones_batch_device(C.byref(self.mpc.desc), C.byref(self.mpc.sp),
                                                               self.mpc.params.ref() if self.mpc.params is not None else None, C.byref(self._est),
                                                               P(self.y_meas), P(self.x_proj), P(self.prev_input()), 2 * self.N, P(self.finished),
                                                               P(self.est_x), P(self.est_P), P(self.est_count), P(self.x0_est), P(self.est_innov),
                                                               P(self.est_nis), None, None, None, C.byref(self._cone_map), self.cones.k_max, self._cone_r,
                                                               P(self.cone_n), P(self.cone_id), P(self.cone_z), P(self.cone_innov), P(self.est_rows), None,
                                                               self._stream(stream)),
                  "fsaempc_cl_estimate_cones_batch_device")
        elif self.estimator is not None:
            check(lib().fsaempc_cl_estimate_cart_batch_device(C.byref(self.mpc.desc), C.byref(self.mpc.sp),
                                                              self.mpc.params.ref() if self.mpc.params is not None else None, C.byref(self._est),
                                                              P(self.y_meas), P(self.x_proj), P(self.prev_input()), 2 * self.N, P(self.finished),
                                                              P(self.est_x), P(self.est_P), P(self.est_count), P(self.x0_est), P(self.est_innov),
                                                              P(self.est_nis), None, None, None, self._stream(stream)),
                  "fsaempc_cl_estimate_cart_batch_device")
        if self.estimator is not None:
            state = self.x0_est
            if self.latency is not None and self.latency.compensate:
                self._observe_call(self._lat_pred, self.x0_est, self._obs_scratch, self.x0_mpc, stream)
                state = self.x0_mpc
        elif self.latency is not None:   # (no sigma next to sensors: x0_obs is a copy of x_proj, x0_mpc its prediction)
            self._observe_call(self._lat, self.x_proj, self.x0_obs, self.x0_mpc, stream)
            state = self.x0_mpc
        self._reference_from(state, stream)
        return state

    def _nmpc_step(self, x0, stream):
        """Shift, SQP and take-over of one period under an Nmpc controller; x0: the state the solve reads."""
        torch, c = self.torch, self.controller
        st = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        nmpc_shift(self.u_opt, self.finished if c.skip_finished else None, 0 if self.steps == 0 else 1, self.u_init, self.nmpc_skip, st)
        # (the call blocks once per sweep: it reads the number of cars still in the sub-batch)
        res = self.sqp.solve(x0, self.x_ref, self.u_init, stream=st, skip=self.nmpc_skip, max_sweeps=c.sweeps, **c.sqp_opts)
        self.nmpc_status = res["status"]
        exitflag = torch.empty(self.B, dtype=torch.int32, device=self.device)
        it = torch.empty(self.B, dtype=torch.int32, device=self.device)
        nmpc_accept(self.model, self.N, res["x_opt"], res["u_opt"], res["status"], res["qp_iter"], self.nmpc_skip, self.x_opt, self.u_opt, exitflag, it, st)
        return dict(x_opt=res["x_opt"], u_opt=res["u_opt"], slack=res["slack"], fval=res["fval"], exitflag=exitflag, iter=it, status=res["status"],
                    sweeps=res["sweeps"], qp_iter=res["qp_iter"], step_norm=res["step_norm"], hard_viol=res["hard_viol"])

    def step(self, stream=None):
        torch = self.torch
        self.pre(stream)
        if self.laps > 1:
            self.lap_gate(stream)
        x_init = None
        if self.warm_start and self.steps > 0:
            N = self.N
            x_init = self._x_init
            nu = 2 * self.mpc.n_blocks
            if self.mpc.blocking is not None:
                # held inputs: the shifted previous plan (u_2 .. u_N, u_N) sampled at each block's first step
                x_init[:, :nu].view(self.B, nu // 2, 2).copy_(self.u_opt[:, self._shift_idx, :])
            else:
                x_init[:, : 2 * (N - 1)].view(self.B, N - 1, 2).copy_(self.u_opt[:, 1:, :])   # (no temporaries: strided views on both sides)
                x_init[:, 2 * (N - 1): 2 * N].copy_(self.u_opt[:, N - 1, :])
            if self._slack is not None:
                x_init[:, nu:].copy_(self._slack)
        x0 = self.x0
        if self.sensors is not None:
            x0 = self.sensed_state(stream)
        elif self.estimator is not None:
            x0 = self.estimate(stream)
        elif self.latency is not None:
            self.observe(stream)
            x0 = self.x0_mpc
        P = lambda t: C.c_void_p(t.data_ptr())
        if self.controller is not None:
            out = self._nmpc_step(x0, stream)
        else:
            out = self.mpc.step(x0, self.x_ref, self.x_opt, self.u_opt, stream=stream, x_init=x_init,
                                difficulty=self._last_iter if self.launch_hint else None)   # linearised about the previous plan (main.m:121-125)
            if self.warm_start:
                self._slack = out["slack"]
            self._last_iter = out["iter"]
            check(lib().fsaempc_cl_accept_batch_device(self.model, self.N, self.B, P(out["x_opt"]), P(out["u_opt"]), P(out["exitflag"]), P(self.x_opt), P(self.u_opt),
                                                       self._stream(stream)), "fsaempc_cl_accept_batch_device")
        if self.u_hist is not None:   # the newest plan into its slot, the plant on the one accepted `delay` periods ago
            d = self.latency.delay
            self.x_hist[self.steps % (d + 1)].copy_(self.x_opt)
            self.u_hist[self.steps % (d + 1)].copy_(self.u_opt)
            self.plant_plan = self.x_hist[(self.steps - d) % (d + 1)]
            self.plant(None, stream, self.plant_plan)
        else:
            self.plant(None, stream)
        if self.metrics is not None:
            check(lib().fsaempc_cl_metrics_batch_device_c(self.model, self.N, C.c_double(self.dt), C.c_double(self.slack_tol), self.B,
                                                          self.mpc.params.ref() if self.mpc.params is not None else None,
                                                          self.corridor.ref() if self.corridor is not None else None,
                                                          P(self.x0), P(self.finished), P(out["exitflag"]), P(out["iter"]), P(out["fval"]),
                                                          P(out["slack"]), P(self.u_opt), P(self.cart), P(self.metrics), self._stream(stream)),
                  "fsaempc_cl_metrics_batch_device_c")
        self.steps += 1
        return out

    def report(self):
        """The lap report so far (LapReport): one read-back of self.metrics."""
        if self.metrics is None:
            raise ValueError("ClosedLoop(metrics=True) keeps the records report() reads")
        if self.lap_records is None:
            return LapReport(self.metrics.cpu().numpy(), self.dt)
        return LapReport(self.metrics.cpu().numpy(), self.dt, self.lap_times.cpu().numpy(), self.lap_state.cpu().numpy(), self.lap_records.cpu().numpy())


def monte_carlo_carts(track, B, seed, lap=False):
    """Initial Cartesian states of BASELINE configs[3]: s0 = u*L, lateral +-0.5 m, heading +-0.1 rad,
    speed U[0,15]; numpy PCG64(seed).  lap: every car at s = 0 and at rest instead (main.m:63 starts from zeros(7,1)), same lateral and
    heading scatter.  Returns (cart (B,7), s0 (B,))."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, track.L, B); n = rng.uniform(-0.5, 0.5, B); dth = rng.uniform(-0.1, 0.1, B); v = rng.uniform(0, 15, B)
    if lap:
        s = np.zeros(B); v = np.zeros(B)

    def ev(P, t):   # the Bezier table on the host (same formulas as interpolate_spline / interpolate_spline_d); P is M x 4
        r = np.mod(t, track.dl * track.M); i = np.minimum(np.floor(r / track.dl).astype(int), track.M - 1); u = r / track.dl - i; w = 1 - u
        val = P[i, 0] * w ** 3 + 3 * P[i, 1] * w * w * u + 3 * P[i, 2] * w * u * u + P[i, 3] * u ** 3
        d = (-3 * w * w * P[i, 0] + 3 * (3 * u * u - 4 * u + 1) * P[i, 1] + 3 * (2 * u - 3 * u * u) * P[i, 2] + 3 * u * u * P[i, 3]) / track.dl
        return val, d
    x, xd = ev(track.xP, s); y, yd = ev(track.yP, s)
    nrm = np.hypot(xd, yd)
    cart = np.zeros((B, 7))
    cart[:, 0] = x - yd / nrm * n; cart[:, 1] = y + xd / nrm * n; cart[:, 2] = np.arctan2(yd, xd) + dth; cart[:, 3] = v
    return cart, s


def monte_carlo(model, N, track, B, steps, seed=20190, options=None, device="cuda:0", warm_start=False, launch_hint=True, params=None,
                plant_params=None, blocking=None, reference=None, metrics=False, corridor=None, laps=1, latency=None, estimator=None, controller=None, sensors=None,
                cones=None):
    """Closed-loop Monte-Carlo: B cars from random initial states, `steps` receding-horizon steps, device-resident loop.
    reference: None (the live ramp) or a Plan the cars track (ClosedLoop).  metrics: ClosedLoop(metrics=True); cl.report() afterwards.
    corridor: None or a Corridor (ClosedLoop).  laps: ClosedLoop(laps=...); cl.lap_times afterwards.  latency: None or a Latency (ClosedLoop).  estimator: None or an Estimator (ClosedLoop).
    sensors: None or a CartesianSensors (ClosedLoop).  cones: None or a ConeSensor (ClosedLoop).
    controller: None (the LTV-MPC step) or an Nmpc (ClosedLoop; the tallies are then the take-over's exit flags and the SQP's QP iterations).
    Returns the ClosedLoop and the per-step tallies (exit flags, iteration counts, driving mask), read back once at the end --
    the reference reports exactly this tally as "abnormal exits %" (main.m:209,222)."""
    import torch
    cart0, s_init = monte_carlo_carts(track, B, seed)
    cl = ClosedLoop(model, N, 0.05, track, cart0, options=options, device=device, warm_start=warm_start, launch_hint=launch_hint,
                    params=params, plant_params=plant_params, blocking=blocking, reference=reference, metrics=metrics, corridor=corridor, laps=laps,
                    latency=latency, estimator=estimator, controller=controller, sensors=sensors, cones=cones)
    cl.x_opt[:, :, 0] += torch.from_numpy(s_init).to(cl.device)[:, None]        # start the closest-point search near the car
    cl.x_opt[:, :, 3] += torch.from_numpy(cart0[:, 3]).to(cl.device)[:, None]   # and the first linearisation at its speed
    flags = torch.zeros((steps, B), dtype=torch.int32, device=cl.device)
    iters = torch.zeros((steps, B), dtype=torch.int32, device=cl.device)
    active = torch.zeros((steps, B), dtype=torch.bool, device=cl.device)
    for t in range(steps):
        out = cl.step()
        flags[t] = out["exitflag"]; iters[t] = out["iter"]; active[t] = cl.finished == 0
    torch.cuda.synchronize(cl.device)
    return cl, flags.cpu().numpy(), iters.cpu().numpy(), active.cpu().numpy()
