"""s-varying track corridors: the two edges of the track as periodic tables over arc length, in place of the one
width N_MAX.  `Corridor.from_table` takes a user's own tables, `Corridor.constant` a band of fixed half-width, `Corridor.from_cones`
derives the tables from the cones that mark the track, on the device.  A Corridor goes to LtvBatch / ClosedLoop /
monte_carlo (`corridor=`: the MPC's track rows and the lap report's track violation) and to Plan.raceline (the box of every control
point, or with rows="cells" one constraint row per cell).
The limits are for the car's reference point: the caller subtracts the half-width of the car."""
import ctypes as C
import math

import numpy as np

from ._lib import CONE_INFO_INDEX, CONES_MAX, NCONEINFO, ConeMaps, CorridorTable, Spline, check, lib

_check = check   # (from_cones has a parameter of that name)


def _host(a, name):
    if hasattr(a, "detach"):   # a torch tensor, wherever it lives
        a = a.detach().cpu().numpy()
    try:
        return np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("%s must be an array of (N_w,) or (P, N_w) numbers" % name)


def check_tables(n_lo, n_hi, L):
    """Validates a corridor's tables on the host (no library call); returns (n_lo, n_hi) as (P, N_w) float64 arrays."""
    lo, hi = _host(n_lo, "n_lo"), _host(n_hi, "n_hi")
    if lo.shape != hi.shape:
        raise ValueError("corridor shapes disagree: n_lo %s, n_hi %s" % (lo.shape, hi.shape))
    if lo.ndim not in (1, 2) or lo.shape[-1] < 2 or (lo.ndim == 2 and lo.shape[0] < 1):
        raise ValueError("corridor tables must be (N_w,) or (P, N_w) with N_w >= 2, got %s" % (lo.shape,))
    if not (isinstance(L, (int, float, np.floating, np.integer)) and math.isfinite(L) and L > 0):
        raise ValueError("L must be finite and > 0, got %r" % (L,))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("corridor tables must be finite")
    if not (lo < hi).all():
        bad = np.argwhere(~(lo < hi))[0]
        raise ValueError("corridor: n_lo < n_hi must hold in every cell (fails at %s: n_lo = %r, n_hi = %r)"
                         % (tuple(int(v) for v in bad), float(lo[tuple(bad)]), float(hi[tuple(bad)])))
    return lo.reshape(-1, lo.shape[-1]), hi.reshape(-1, hi.shape[-1])


class Corridor:
    """P corridors of N_w cells on the device: n_lo, n_hi (P, N_w), cell i at s_i = i ds, ds = L / N_w, periodic and linear in
    between.  P = 1: shared by every car / plan; otherwise car (plan) b has corridor b."""

    def __init__(self, n_lo, n_hi, L):
        self.n_lo, self.n_hi, self.L = n_lo, n_hi, float(L)
        self.P, self.N_w = int(n_lo.shape[0]), int(n_lo.shape[1])
        self.ds = self.L / self.N_w
        self.device = n_lo.device
        self.info = None   # from_cones(check=True): the (P, 8) info block of the cone stage
        self.c = CorridorTable(C.c_void_p(n_lo.data_ptr()), C.c_void_p(n_hi.data_ptr()), self.N_w, self.ds, 1 if self.P > 1 else 0)

    def ref(self):
        return C.byref(self.c)

    @staticmethod
    def from_table(n_lo, n_hi, L, device="cuda:0"):
        """n_lo, n_hi: (N_w,) or (P, N_w), numpy arrays or tensors; L the lap length the N_w cells cover.  Validated on the host
        before anything else: equal shapes, N_w >= 2, finite entries, n_lo < n_hi in every cell."""
        lo, hi = check_tables(n_lo, n_hi, L)
        import torch
        dev = torch.device(device)
        up = lambda a: torch.from_numpy(a).to(device=dev, dtype=torch.float64).contiguous()
        return Corridor(up(lo), up(hi), L)

    @staticmethod
    def constant(L, half_width, N_w=2, device="cuda:0"):
        """The band -half_width .. +half_width all round the lap (half_width = N_MAX gives the bits of the calls without a corridor)."""
        if not (isinstance(half_width, (int, float, np.floating, np.integer)) and math.isfinite(half_width) and half_width > 0):
            raise ValueError("half_width must be finite and > 0, got %r" % (half_width,))
        if int(N_w) != N_w or N_w < 2:
            raise ValueError("N_w must be an integer >= 2, got %r" % (N_w,))
        return Corridor.from_table(np.full(int(N_w), -float(half_width)), np.full(int(N_w), float(half_width)), L, device=device)

    @staticmethod
    def from_cones(track, left, right, N_w, margin=0.0, reach=5.0, device="cuda:0", stream=None, check=True):
        """The corridor of a track from the two rows of cones that mark it, on the device (fsaempc_corridor_from_cones_device,
        DESIGN.md 6n).  left, right: (K, 2) for one corridor or (P, K, 2) for P of them (a batch on one side, one map on the other:
        the one map is repeated), numpy arrays or device tensors; a cone with a NaN coordinate is absent, which pads maps of
        different sizes.  margin: taken off both edges (the car's half-width); reach: cones further from the line are strays.
        Returns a Corridor whose .info is the (P, 8) host array of CONE_INFO_INDEX.  check=True reads the info once and raises
        ValueError, naming the corridor and the reason, when a side kept no cone or a cell has no room (n_lo < n_hi fails);
        check=False synchronises nothing and leaves .info None."""
        import torch
        dev = torch.device(device)
        if int(N_w) != N_w or N_w < 2:
            raise ValueError("N_w must be an integer >= 2, got %r" % (N_w,))
        sides = []
        for a, name in ((left, "left"), (right, "right")):
            if not isinstance(a, torch.Tensor):
                try:
                    a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
                except (TypeError, ValueError):
                    raise ValueError("%s must be an array of (K, 2) or (P, K, 2) numbers" % name)
            if a.dim() not in (2, 3) or a.shape[-1] != 2 or (a.dim() == 3 and a.shape[0] < 1):
                raise ValueError("%s must be (K, 2) or (P, K, 2), got %s" % (name, tuple(a.shape)))
            if a.shape[-2] > CONES_MAX:
                raise ValueError("%s holds %d cones per map, at most %d are supported" % (name, a.shape[-2], CONES_MAX))
            sides.append(a.to(device=dev, dtype=torch.float64))
        counts = {int(a.shape[0]) for a in sides if a.dim() == 3}
        if len(counts) > 1:
            raise ValueError("left and right hold different numbers of maps: %s and %s" % (tuple(sides[0].shape), tuple(sides[1].shape)))
        P = counts.pop() if counts else 1
        per = 1 if any(a.dim() == 3 for a in sides) else 0
        if per:
            sides = [a if a.dim() == 3 else a.unsqueeze(0).expand(P, -1, -1) for a in sides]
        le, ri = (a.contiguous() for a in sides)
        xP, yP = track.device(dev)
        sp = Spline(track.M, track.dl, C.c_void_p(xP.data_ptr()), C.c_void_p(yP.data_ptr()))
        maps = ConeMaps(C.c_void_p(le.data_ptr() if le.numel() else None), C.c_void_p(ri.data_ptr() if ri.numel() else None),
                        int(le.shape[-2]), int(ri.shape[-2]), per)
        n_lo = torch.empty((P, int(N_w)), dtype=torch.float64, device=dev)
        n_hi = torch.empty_like(n_lo)
        info = torch.empty((P, NCONEINFO), dtype=torch.float64, device=dev) if check else None
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
        _check(lib().fsaempc_corridor_from_cones_device(C.byref(sp), C.c_double(track.L), C.byref(maps), P, int(N_w), C.c_double(margin),
                                                        C.c_double(reach), C.c_void_p(n_lo.data_ptr()), C.c_void_p(n_hi.data_ptr()),
                                                        C.c_void_p(info.data_ptr() if check else None), st),
               "fsaempc_corridor_from_cones_device")
        cor = Corridor(n_lo, n_hi, track.L)
        cor._cones = (le, ri)   # (the launch is asynchronous: the maps live as long as the tables)
        if check:
            if stream is not None:
                torch.cuda.synchronize(dev)        # (a raw stream handle: the copy below orders itself on torch's current stream only)
            cor.info = info.cpu().numpy()
            for p, row in enumerate(cor.info):
                for slot, side in ((CONE_INFO_INDEX["KEPT_LEFT"], "left"), (CONE_INFO_INDEX["KEPT_RIGHT"], "right")):
                    if row[slot] == 0:
                        raise ValueError("corridor %d: no %s cone was kept (absent %d, unprojected %d, beyond reach %d over both sides)"
                                         % (p, side, row[2], row[3], row[4]))
                if row[CONE_INFO_INDEX["CELLS_NO_ROOM"]] != 0:
                    raise ValueError("corridor %d: n_lo < n_hi fails in %d cells (least width %r with margin %r)"
                                     % (p, row[6], float(row[7]), float(margin)))
        return cor

    def line_bounds(self, N_s, N_c, margin, n_plans=None, stream=None):
        """(lb, ub), each (n_plans, N_c) on the device: the bounds Plan.raceline(corridor=self) hands to the line QP
        (fsaempc_corridor_line_bounds_device); NaN where the corridor leaves a control point no box.  n_plans: default the corridor's
        own count."""
        import torch
        n_plans = self.P if n_plans is None else int(n_plans)
        self.check_batch(n_plans)
        lb = torch.empty((n_plans, int(N_c)), dtype=torch.float64, device=self.device)
        ub = torch.empty_like(lb)
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream)
        check(lib().fsaempc_corridor_line_bounds_device(self.ref(), C.c_double(self.L), n_plans, int(N_s), int(N_c), C.c_double(margin),
                                                        C.c_void_p(lb.data_ptr()), C.c_void_p(ub.data_ptr()), st),
              "fsaempc_corridor_line_bounds_device")
        return lb, ub

    def line_rows(self, N_s, N_c, margin, n_plans=None, stream=None):
        """(A, lbA, ubA) on the device: the cell-wise rows Plan.raceline(corridor=self, rows="cells") hands to the line QP
        (fsaempc_corridor_line_rows_device).  A (N_c, N_s) is the memory of the column-major N_s x N_c matrix, A[k, i] the weight of
        control point k in the offset at cell i, one for the batch; lbA, ubA (n_plans, N_s), NaN where a cell has no room.  n_plans:
        default the corridor's own count."""
        import torch
        n_plans = self.P if n_plans is None else int(n_plans)
        self.check_batch(n_plans)
        A = torch.empty((int(N_c), int(N_s)), dtype=torch.float64, device=self.device)
        lbA = torch.empty((n_plans, int(N_s)), dtype=torch.float64, device=self.device)
        ubA = torch.empty_like(lbA)
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream)
        check(lib().fsaempc_corridor_line_rows_device(self.ref(), C.c_double(self.L), n_plans, int(N_s), int(N_c), C.c_double(margin),
                                                      C.c_void_p(A.data_ptr()), C.c_void_p(lbA.data_ptr()), C.c_void_p(ubA.data_ptr()), st),
              "fsaempc_corridor_line_rows_device")
        return A, lbA, ubA

    def check_batch(self, B):
        if self.P not in (1, B):
            raise ValueError("the corridor holds %d tables: it serves a batch of %d (one per car) or any batch (one shared), not %d"
                             % (self.P, self.P, B))

    def check_device(self, device):
        """The corridor lives on one device; what reads it must run there (compared by name, before any device call)."""
        want, have = str(device), str(self.device)
        if want.split(":")[0] != have.split(":")[0] or (":" in want and ":" in have and want != have):
            raise ValueError("the corridor is on %s, the caller on %s" % (have, want))


def check_corridor(corridor, B, device):
    """None or a Corridor that serves a batch of B on `device` (no library call)."""
    if corridor is None:
        return None
    if not isinstance(corridor, Corridor):
        raise ValueError("corridor must be None or a Corridor")
    corridor.check_batch(B)
    corridor.check_device(device)
    return corridor
