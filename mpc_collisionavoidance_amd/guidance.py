"""Batched counterpart of the reference's obstacle-avoidance ROS node around the solver
(class NMPC, /root/reference/catkin_ws/src/nmpc_ca/src/nmpc_guidance_ca1.cpp): waypoint manager,
LiDAR obstacle selection / body->NED transform, x0 assembly, and the published set-points.  All
arithmetic runs on the device (csrc/ca_guidance.hpp); this class only moves arrays.  Two ways to drive it:

    host-fed          sense(pose, world) -> prepare(vel_uv, pose) -> solve -> publish()       (the ROS nodes' callbacks)
    device-resident   set_world(world) once; prepare() -> solve_async -> publish(fetch=False) -> advance / advance_sim
                      the vessel's state is read from the solver's own x0; no host array, no synchronisation"""
import ctypes as C

import numpy as np

from . import _capi


class _ResidentWorld:
    """What the two front ends share: the world list that lives on the device (csrc/world_plan.hpp holds its rules for both).  A subclass
    names its C symbols - usvmpc_<_prefix>_world, _world_vel, _world_step, _world_read, _fleet, _fleet_state - and keeps its own set_world,
    whose arguments differ.  Attributes: s (the solver), B, _lib; _L (fixed entries of the list, once set) and _S (scene size, a fleet on)."""
    _prefix = None

    def _world_call(self, name, *args):
        self.s._check(getattr(self._lib, "usvmpc_%s_%s" % (self._prefix, name))(self.s._h, *args))

    def _world_arrays(self, world, vel):
        """set_world's arrays, checked: (world [B, L, 3], vel [B, L, 2] or None); a fleet's world moves, so vel None is zeros then"""
        S = getattr(self, "_S", 0)
        w = _as_world(world, self.B, 64 - (S - 1 if S else 0))
        v = None if vel is None else _as_world_vel(vel, self.B, w.shape[1])
        if S and v is None:
            v = np.zeros((self.B, w.shape[1], 2))
        return w, v

    def _upload_world(self, w, v, max_radius, *vel_args):
        self._world_call("world", w.ctypes.data_as(_capi._dp) if w.size else None, w.shape[1], float(max_radius))
        self._world_call("world_vel", None if v is None else v.ctypes.data_as(_capi._dp), *vel_args)
        self._L = w.shape[1]

    def set_fleet(self, scene_size, radius=0.5, plans=False):
        """Vessel encounters: the batch is cut into scenes of scene_size = S consecutive instances, and every instance sees the other
        S - 1 vessels of its scene - position, hull radius `radius`, velocity from the state the plant left in x0 (the guidance model: (u, v)
        turned by psi) - as moving world entries behind its fixed ones (set_world), refreshed on the device by every device-resident
        prepare().  B % S == 0; after reset() and set_world() (an empty world will do).  GuidanceFrontEnd: over a world at rest the scene is
        predicted per stage; a set_world(..., predict=False) AFTER this call holds it still inside the horizon.  scene_size 0 or 1: off, the
        world list is the fixed entries again.
        plans=True (exchanged plans, csrc/fleet_plan.hpp; N >= 2): a scene-mate's slot follows the path the mate's own NMPC has just
        solved, x[j][1 .. N] moved by what the plant did to the mate since, instead of the straight line pos + (k dt) vel - whenever the
        iterate is exactly one hand-over old (solve -> advance / advance_sim -> prepare), the mate's mission is not over and its last solve
        succeeded; every other slot, and every prepare in any other state, keeps the constant-velocity stages.  fleet_plan_state() tells which
        slots were fed."""
        self._world_call("fleet", int(scene_size), float(radius))
        self._S = int(scene_size) if int(scene_size) >= 2 else 0
        if self._S and (plans or getattr(self, "_plans", False)):
            self._world_call("fleet_plans", 1 if plans else 0)
            self._plans = bool(plans)

    def fleet_plan_state(self):
        """dict(source [B, K] (the vessel whose plan fed each slot at the last prepare; -1: none - the slot kept its constant-velocity stages),
        plan_fed (plan-fed (instance, slot) pairs so far, counted on the device), plan_launches (launches of the plan kernel so far))."""
        src = np.full((self.B, self.s.K), -1, dtype=np.int32)
        fed, launches = C.c_longlong(0), C.c_longlong(0)
        self._world_call("fleet_plan_state", src.ctypes.data_as(_capi._ip), C.byref(fed), C.byref(launches))
        return dict(source=src, plan_fed=int(fed.value), plan_launches=int(launches.value))

    def fleet_state(self):
        """dict(min_separation [B] (smallest distance to a vessel of the instance's scene, any tick; 1e300 before the first),
        separation_tick [B] (the prepare it was met at; -1: none yet))."""
        ms, st = np.zeros(self.B), np.zeros(self.B, dtype=np.int32)
        self._world_call("fleet_state", ms.ctypes.data_as(_capi._dp), st.ctypes.data_as(_capi._ip))
        return dict(min_separation=ms, separation_tick=st)

    def step_world(self, T):
        """The world moves on by T seconds (enqueued; a moving world only)."""
        self._world_call("world_step", float(T))

    def world(self):
        """(world [B, L, 3], vel [B, L, 2]) as the device holds them; vel is zero for a world at rest.  While a fleet is on L counts the
        fixed entries and the S - 1 fleet entries behind them."""
        L = getattr(self, "_L", None)
        if L is None:
            raise Exception("world: no world list yet (set_world first)")
        S = getattr(self, "_S", 0)
        L += S - 1 if S else 0
        w, v = np.zeros((self.B, L, 3)), np.zeros((self.B, L, 2))
        self._world_call("world_read", w.ctypes.data_as(_capi._dp), v.ctypes.data_as(_capi._dp))
        return w, v


class GuidanceFrontEnd(_ResidentWorld):
    _prefix = "guidance"

    def __init__(self, solver):
        if solver.ocp.model.name != "usv_model_guidance_ca1":
            raise Exception("the guidance front end belongs to usv_model_guidance_ca1")
        self.s = solver
        self.B = solver.B
        self._lib = solver._lib

    def reset(self, waypoints, psi):
        """New waypoint list: waypoints [B, npts, 2] (or [npts, 2] for all), psi [B]."""
        w = np.ascontiguousarray(waypoints, dtype=np.float64)
        if w.ndim == 2:
            w = np.tile(w[None], (self.B, 1, 1))
        w = np.ascontiguousarray(w.reshape(self.B, -1))
        psi = np.ascontiguousarray(np.broadcast_to(np.asarray(psi, dtype=np.float64), (self.B,)))
        self.s._check(self._lib.usvmpc_guidance_reset(self.s._h, w.ctypes.data_as(_capi._dp), w.shape[1] // 2,
                                                      psi.ctypes.data_as(_capi._dp)))

    def sense(self, pose, world, max_radius=100.0, fetch=False):
        """The obstacle simulator's simulate(): world [B,L,3] (or [L,3] for all) NED (X, Y, R), pose [B,3]
        (nedx, nedy, yaw).  The visible obstacles, in the body frame, stay on the device for the next
        prepare(..., obstacles=None); fetch=True also returns (obstacles [B,64,3], n [B])."""
        p = np.ascontiguousarray(pose, dtype=np.float64).reshape(self.B, 3)
        w = np.asarray(world, dtype=np.float64)
        if w.ndim == 2:
            w = np.tile(w[None], (self.B, 1, 1))
        w = np.ascontiguousarray(w.reshape(self.B, -1, 3))
        o = np.zeros((self.B, 64, 3)) if fetch else None
        n = np.zeros(self.B, dtype=np.int32) if fetch else None
        self.s._check(self._lib.usvmpc_guidance_sense(self.s._h, p.ctypes.data_as(_capi._dp), w.ctypes.data_as(_capi._dp),
                                                      w.shape[1], float(max_radius),
                                                      o.ctypes.data_as(_capi._dp) if fetch else None,
                                                      n.ctypes.data_as(_capi._ip) if fetch else None))
        return (o, n) if fetch else None

    def set_world(self, world, max_radius=100.0, vel=None, predict=True):
        """The obstacle field (X, Y, R) in NED for the device-resident mode: [B, L, 3] or [L, 3] for all, L <= 64; uploaded once.
        vel: [B, L, 2] or [L, 2] (vX, vY) in NED m/s - the world moves: advance / advance_sim move it along (option
        "obstacle_step_on_advance") and, with predict, prepare() writes the predicted obstacle set of every stage; predict=False holds the
        world still inside the horizon (stage 0 only).  None: a world at rest.
        While a fleet is on (set_fleet) these are the FIXED entries, L <= 64 - (S - 1): the fleet's slots stay behind them, and vel None
        gives the fixed entries zero velocities (the scene's world moves)."""
        self._upload_world(*self._world_arrays(world, vel), max_radius, 1 if predict else 0)

    def prepare(self, vel_uv=None, pose=None, obstacles=None, n_obstacles=None):
        """vel_uv [B,2], pose [B,3] (nedx, nedy, psi), obstacles [B,L,3] body (x, y, R), n_obstacles [B];
        obstacles=None: the lists sense() left on the device.  vel_uv and pose both None: device-resident - the vessel's state is read
        from the solver's own x0 and the obstacles from the world of set_world(); enqueues and returns."""
        if (vel_uv is None) != (pose is None):
            raise Exception("prepare: give both vel_uv and pose, or neither")
        if vel_uv is None:
            self.s._check(self._lib.usvmpc_guidance_prepare(self.s._h, None, None, None, None, 0))
            return
        v = np.ascontiguousarray(vel_uv, dtype=np.float64).reshape(self.B, 2)
        p = np.ascontiguousarray(pose, dtype=np.float64).reshape(self.B, 3)
        if obstacles is None:
            self.s._check(self._lib.usvmpc_guidance_prepare(self.s._h, v.ctypes.data_as(_capi._dp), p.ctypes.data_as(_capi._dp),
                                                            None, None, 0))
            return
        o = np.ascontiguousarray(obstacles, dtype=np.float64).reshape(self.B, -1, 3)
        n = np.ascontiguousarray(n_obstacles, dtype=np.int32).reshape(self.B)
        self.s._check(self._lib.usvmpc_guidance_prepare(self.s._h, v.ctypes.data_as(_capi._dp), p.ctypes.data_as(_capi._dp),
                                                        o.ctypes.data_as(_capi._dp), n.ctypes.data_as(_capi._ip), o.shape[1]))

    def publish(self, fetch=True):
        """After solve(): dict(heading, r, speed, ye, active) - the node's published set-points.  fetch=False: enqueue only, returns None."""
        if not fetch:
            self.s._check(self._lib.usvmpc_guidance_publish(self.s._h, None, None, None, None, None))
            return None
        h, r, sp, ye = (np.zeros(self.B) for _ in range(4))
        act = np.zeros(self.B, dtype=np.int32)
        self.s._check(self._lib.usvmpc_guidance_publish(self.s._h, h.ctypes.data_as(_capi._dp), r.ctypes.data_as(_capi._dp),
                                                        sp.ctypes.data_as(_capi._dp), ye.ctypes.data_as(_capi._dp),
                                                        act.ctypes.data_as(_capi._ip)))
        return dict(heading=h, r=r, speed=sp, ye=ye, active=act)

    def mission_state(self):
        """dict(wp_index [B], past_psied [B], finish_tick [B] (-1: not finished), min_clearance [B]) of the device-resident mode."""
        k, ft = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        pp = np.zeros(self.B, dtype=np.float32)
        mc = np.zeros(self.B)
        self.s._check(self._lib.usvmpc_guidance_mission_state(self.s._h, k.ctypes.data_as(_capi._ip), pp.ctypes.data_as(C.POINTER(C.c_float)),
                                                              ft.ctypes.data_as(_capi._ip), mc.ctypes.data_as(_capi._dp)))
        return dict(wp_index=k, past_psied=pp, finish_tick=ft, min_clearance=mc)

    def state(self):
        k = np.zeros(self.B, dtype=np.int32)
        pp = np.zeros(self.B, dtype=np.float32)
        self.s._check(self._lib.usvmpc_guidance_state(self.s._h, k.ctypes.data_as(_capi._ip),
                                                      pp.ctypes.data_as(C.POINTER(C.c_float))))
        return k, pp


def _as_waypoints(waypoints, B):
    """[B, npts, 2], [B, 2 npts] or one [npts, 2] list for every instance -> contiguous [B, 2 npts]; npts >= 2."""
    w = np.ascontiguousarray(waypoints, dtype=np.float64)
    if w.ndim == 2 and w.shape[1] == 2:
        # [npts, 2]: one list for all.  (A [B, 2] array cannot be a per-instance list: that would be one point each.)
        w = np.tile(w[None], (B, 1, 1))
    if w.ndim not in (2, 3):
        raise Exception("waypoints: expected [%d, npts, 2] or [npts, 2], got %s" % (B, list(w.shape)))
    if w.shape[0] != B:
        raise Exception("waypoints: expected [%d, npts, 2] or [npts, 2], got %s" % (B, list(w.shape)))
    w = np.ascontiguousarray(w.reshape(B, -1))
    if w.shape[1] % 2 or w.shape[1] < 4:
        raise Exception("waypoints: at least two (x, y) points per instance are needed, got %d values" % w.shape[1])
    if not np.isfinite(w).all():
        raise Exception("waypoints contain NaN or infinity")
    return w


def _as_world(world, B, lmax=64):
    """World obstacles (X, Y, R): [B, L, 3], one [L, 3] list for every instance, or None / empty for no obstacle -> contiguous [B, L, 3]."""
    if world is None:
        return np.zeros((B, 0, 3))
    w = np.asarray(world, dtype=np.float64)
    if w.size == 0:
        return np.zeros((B, 0, 3))
    if w.shape[-1] != 3 or w.ndim not in (2, 3):
        raise Exception("world: expected [%d, L, 3] or [L, 3] rows of (X, Y, R), got %s" % (B, list(w.shape)))
    if w.ndim == 2:
        w = np.tile(w[None], (B, 1, 1))
    if w.shape[0] != B:
        raise Exception("world: expected %d instances, got %d" % (B, w.shape[0]))
    if w.shape[1] > lmax:
        raise Exception("world: at most %d obstacles per instance, got %d" % (lmax, w.shape[1]))
    if np.isnan(w).any():
        raise Exception("world contains NaN")
    return np.ascontiguousarray(w)


def _as_world_vel(vel, B, L):
    """World velocities (vX, vY), NED m/s, for a world list of L entries: [B, L, 2] or one [L, 2] list for every instance -> contiguous
    [B, L, 2]."""
    v = np.asarray(vel, dtype=np.float64)
    if v.size == 0 and L == 0:
        return np.zeros((B, 0, 2))
    if v.shape[-1:] != (2,) or v.ndim not in (2, 3):
        raise Exception("world velocities: expected [%d, %d, 2] or [%d, 2] rows of (vX, vY), got %s" % (B, L, L, list(v.shape)))
    if v.ndim == 2:
        v = np.tile(v[None], (B, 1, 1))
    if v.shape[0] != B:
        raise Exception("world velocities: expected %d instances, got %d" % (B, v.shape[0]))
    if v.shape[1] != L:
        raise Exception("world velocities: the world list has %d obstacles per instance, got %d velocities" % (L, v.shape[1]))
    if not np.isfinite(v).all():
        raise Exception("world velocities contain NaN or infinity")
    return np.ascontiguousarray(v)


class PathFollowingFrontEnd(_ResidentWorld):
    """Batched counterpart of the reference's path-following ROS node around the solver (class NMPC,
    catkin_ws/src/nmpc_ca/src/nmpc_pf.cpp = nmpc_pf_ca.cpp) for usv_model_pf_ca: waypoint manager, x0 and reference assembly, nearest-K
    obstacle selection, published thrusts.  The arithmetic runs on the device (csrc/pf_guidance.hpp).  Two ways to drive it:

        host-fed          prepare(vel_uvr, pose) -> solve -> publish()         (the ROS node's callbacks)
        device-resident   prepare() -> solve_async -> publish(fetch=False) -> advance / advance_sim
                          the vessel's state is read from the solver's own x0; no host array, no synchronisation
    """

    _prefix = "pf"

    def __init__(self, solver):
        if solver.ocp.model.name != "usv_model_pf_ca" or getattr(solver, "generated", False):
            raise Exception("the path-following front end belongs to usv_model_pf_ca (this solver's model: %s)" % solver.ocp.model.name)
        self.s = solver
        self.B = solver.B
        self._lib = solver._lib

    def reset(self, waypoints):
        """New waypoint list: [B, npts, 2] (or [npts, 2] for all).  k = 1, past thrust 0; the solver switches to static obstacles."""
        w = _as_waypoints(waypoints, self.B)
        self.s._check(self._lib.usvmpc_pf_reset(self.s._h, w.ctypes.data_as(_capi._dp), w.shape[1] // 2))

    def set_world(self, world, max_radius=100.0, margin=None, vel=None):
        """The obstacle field (X, Y, R) in NED: [B, L, 3] or [L, 3] for all, L <= 64; uploaded once.  margin: lh = (R + 0.5) + margin.
        vel: [B, L, 2] or [L, 2] (vX, vY) in NED m/s - the world moves: prepare() writes the predicted obstacle set of every stage and
        advance / advance_sim move the world along (option "obstacle_step_on_advance").  None: a world at rest.
        While a fleet is on (set_fleet) these are the FIXED entries, L <= 64 - (S - 1): the fleet's slots stay behind them, and vel None
        gives the fixed entries zero velocities (the scene's world moves)."""
        w, v = self._world_arrays(world, vel)
        if margin is not None:
            self.s.set_option("pf_lh_margin", float(margin))
        self._upload_world(w, v, max_radius)

    def prepare(self, vel_uvr=None, pose=None):
        """vel_uvr [B,3] = (u, v, r), pose [B,3] = (nedx, nedy, psi); both None: device-resident (enqueues and returns)."""
        if (vel_uvr is None) != (pose is None):
            raise Exception("prepare: give both vel_uvr and pose, or neither")
        if vel_uvr is None:
            self.s._check(self._lib.usvmpc_pf_prepare(self.s._h, None, None))
            return
        v = _as_rows(vel_uvr, self.B, "vel_uvr")
        p = _as_rows(pose, self.B, "pose")
        self.s._check(self._lib.usvmpc_pf_prepare(self.s._h, v.ctypes.data_as(_capi._dp), p.ctypes.data_as(_capi._dp)))

    def publish(self, fetch=True):
        """After the solve: dict(thr_port, thr_stbd, Tx, Tz, e_u, e_ye, speed, active).  fetch=False: enqueue only, returns None."""
        if not fetch:
            self.s._check(self._lib.usvmpc_pf_publish(self.s._h, None, None, None, None, None, None, None, None))
            return None
        port, stbd, tx, tz, sp = (np.zeros(self.B) for _ in range(5))
        eu, eye = np.zeros(self.B, dtype=np.float32), np.zeros(self.B, dtype=np.float32)
        act = np.zeros(self.B, dtype=np.int32)
        fp = C.POINTER(C.c_float)
        self.s._check(self._lib.usvmpc_pf_publish(self.s._h, port.ctypes.data_as(_capi._dp), stbd.ctypes.data_as(_capi._dp),
                                                  tx.ctypes.data_as(_capi._dp), tz.ctypes.data_as(_capi._dp), eu.ctypes.data_as(fp),
                                                  eye.ctypes.data_as(fp), sp.ctypes.data_as(_capi._dp), act.ctypes.data_as(_capi._ip)))
        return dict(thr_port=port, thr_stbd=stbd, Tx=tx, Tz=tz, e_u=eu, e_ye=eye, speed=sp, active=act)

    def state(self):
        """dict(wp_index [B], finish_tick [B] (-1: not finished), min_clearance [B], yref_writes)."""
        k, ft = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        mc = np.zeros(self.B)
        n = C.c_longlong(0)
        self.s._check(self._lib.usvmpc_pf_state(self.s._h, k.ctypes.data_as(_capi._ip), ft.ctypes.data_as(_capi._ip),
                                                mc.ctypes.data_as(_capi._dp), C.byref(n)))
        return dict(wp_index=k, finish_tick=ft, min_clearance=mc, yref_writes=int(n.value))


def _as_rows(value, B, what):
    a = np.ascontiguousarray(value, dtype=np.float64)
    if a.size != 3 * B:
        raise Exception("%s: expected [%d, 3], got %s" % (what, B, list(a.shape)))
    return np.ascontiguousarray(a.reshape(B, 3))


class Cascade:
    """The two-layer control stack the reference deploys, closed on a vessel with inertia, all on the device (csrc/cascade.hpp; kernels
    usv_cascade_refs, usv_cascade_step): the guidance layer - `front_end`, a device-resident GuidanceFrontEnd after reset() and set_world() -
    publishes a desired heading and speed every `ratio`-th tick (nmpc_guidance_ca1.cpp, 20 Hz); `low_level`, a BatchOcpSolver of
    usv_model_low_level with as many instances (nmpc_low_level.cpp, 100 Hz), turns them into thrusts at every tick; a 3-DOF vessel
    (nedx, nedy, psi, u, v, r) integrates the published thrusts over the low-level shooting interval in num_steps RK4 steps, starboard
    factor c.  ratio * low_level.dt must be the guidance solver's dt.

        tick()   every ratio-th tick first  prepare() -> solve_async() -> publish(fetch=False)  of the guidance layer,
                 then                       refs -> low_level.solve_async() -> step
    No host array and no synchronisation in a tick.  Neither solver's advance is called, so the solvers' own closed-loop logs do not see
    cascade ticks: a cascade's runs are recorded by its own log - start_log() / read_log(), kernel usv_cascade_record ahead of every logged
    step - and costed by track_cost() / tracked_cost(), the realised cost of either layer, both on the device and without synchronising."""

    def __init__(self, front_end, low_level, ratio=5, num_steps=1, c=0.78, instance_offset=0):
        import torch
        if not isinstance(front_end, GuidanceFrontEnd) or getattr(front_end.s, "generated", False):
            raise Exception("Cascade: the upper layer is a GuidanceFrontEnd on a usv_model_guidance_ca1 solver of the stock library")
        if low_level.ocp.model.name != "usv_model_low_level" or (low_level.nx, low_level.nu) != (8, 2):
            raise Exception("Cascade: the lower layer is a solver of usv_model_low_level (this one's model: %s)" % low_level.ocp.model.name)
        if low_level.B != front_end.B:
            raise Exception("Cascade: the two layers need the same batch (guidance %d, low level %d)" % (front_end.B, low_level.B))
        self.fe, self.g, self.ll = front_end, front_end.s, low_level
        self.B, self.ratio = front_end.B, int(ratio)
        self._lib = self.g._lib
        # one stream for both solvers: the kernels of the two libraries are ordered by it and by nothing else
        self._stream = torch.cuda.Stream(device=self.g._desc.device)
        self.g.set_stream(self._stream.cuda_stream)
        self.ll.set_stream(self._stream.cuda_stream)
        # the low-level solver's yref and x0 are written behind its back, through device pointers, by a kernel of another library: every
        # solve must linearise afresh from device memory ("pipeline_linearize" 0: no pass made a tick ahead on the old rows), and no host copy
        # of its arrays may stand in for the device's ("host_mirror" 0: no deferred upload lands on top of what the cascade wrote, no
        # read-back per solve)
        self.ll.set_option("pipeline_linearize", 0)
        self.ll.set_option("host_mirror", 0)
        h = C.c_void_p()
        rc = self._lib.usvmpc_cascade_create(self.g._h, self.ratio, float(self.ll.dt), int(num_steps), float(c), int(instance_offset), self.ll.B,
                                             self.ll.N, *(C.c_void_p(self.ll.device_ptr(f)) for f in ("x0", "x", "yref", "yref_e")), C.byref(h))
        if rc != 0:
            raise Exception(self._lib.usvmpc_cascade_last_error(None).decode())
        self._c = h
        self._t = 0
        self._log = None
        self._track = False

    def _check(self, rc):
        if rc < 0:
            raise Exception(self._lib.usvmpc_cascade_last_error(self._c).decode())
        return rc

    def reset(self, pose, vel):
        """pose [B,3] = (nedx, nedy, psi), vel [B,3] = (u, v, r): the vessel's state.  Past thrusts 0, tick 0, sums 0; the guidance solver's
        x0 gets (u, v) and the pose; the low-level initial iterate becomes x_k = x0 for every k, u = 0."""
        from . import scenario
        p, v = _as_rows(pose, self.B, "pose"), _as_rows(vel, self.B, "vel")
        self._check(self._lib.usvmpc_cascade_reset(self._c, p.ctypes.data_as(_capi._dp), v.ctypes.data_as(_capi._dp)))
        x0, _ = scenario.cascade_ll_inputs(np.column_stack([p, v]), np.zeros((self.B, 2)), np.zeros(self.B), np.zeros(self.B))
        self.ll.set("x0", 0, x0)
        self.ll.set_all("x", np.tile(x0[:, None, :], (1, self.ll.N + 1, 1)))
        self.ll.set_all("u", np.zeros((self.B, self.ll.N, 2)))
        self._t = 0

    def guidance_tick(self):
        """whether the next tick() begins with a guidance solve"""
        return self._t % self.ratio == 0

    def guidance(self):
        """the guidance layer's part of a tick (enqueued)"""
        self.fe.prepare()
        self.g.solve_async()
        if self._track:
            self.g.track_cost_now()
        self.fe.publish(fetch=False)

    def refs(self):
        """kernel usv_cascade_refs (enqueued): the low-level solver's x0 and, where the set-points changed, its reference rows"""
        self._check(self._lib.usvmpc_cascade_refs(self._c))

    def step(self, sigma=0.0, seed=0):
        """kernel usv_cascade_step (enqueued): thrusts from the low-level x_1, one plant period (+ sigma N(0,1) on u, v, r), the hand-over"""
        self._check(self._lib.usvmpc_cascade_step(self._c, float(sigma), int(seed)))
        self._t += 1

    def tick(self, sigma=0.0, seed=0):
        """One low-level tick; enqueues and returns."""
        if self.guidance_tick():
            self.guidance()
        self.refs()
        self.ll.solve_async()
        if self._track:
            self.ll.track_cost_now()
        self.step(sigma, seed)

    def state(self):
        """dict(state [B,6] = (nedx, nedy, psi, u, v, r), thrust [B,2] (published), past_thrust [B,2], ticks [B], yref_writes,
        err_sums [B,4] = (sum |e_u|, sum |e_psi|, sum e_u^2, sum e_psi^2)); waits for the stream."""
        s, th, pa, es = np.zeros((self.B, 6)), np.zeros((self.B, 2)), np.zeros((self.B, 2)), np.zeros((self.B, 4))
        tk = np.zeros(self.B, dtype=np.int32)
        n = C.c_longlong(0)
        self._check(self._lib.usvmpc_cascade_state(self._c, s.ctypes.data_as(_capi._dp), th.ctypes.data_as(_capi._dp), pa.ctypes.data_as(_capi._dp),
                                                   tk.ctypes.data_as(_capi._ip), C.byref(n), es.ctypes.data_as(_capi._dp)))
        return dict(state=s, thrust=th, past_thrust=pa, ticks=tk, yref_writes=int(n.value), err_sums=es)

    # -- the log (include/usvmpc.h, "Cascade log"): states, thrusts, set-points, errors and both layers' status kept on the device
    STATES = ("nedx", "nedy", "psi", "u", "v", "r")

    def start_log(self, capacity, every=1, first=0, states=None, thrust=True, ref=True, err=False, status=True):
        """From now on every step (a low-level tick, counted from 0) first records, on the device and without synchronising: tick i makes a
        record when i >= first, (i - first) % every == 0 and fewer than `capacity` exist.  states: None (all six) or a list of indices into
        (nedx, nedy, psi, u, v, r) (stored in ascending order; an empty list: no state channel) - the vessel's state as the tick's low-level
        solve saw it; thrust: the two thrusts the tick publishes; ref: the (heading, speed) the low level tracks; err: (e_u, e_psi) as
        float32; status: status and qp_iter of both layers' last solves."""
        d = _capi.CascadeLogDesc()
        d.capacity, d.every, d.first = int(capacity), int(every), int(first)
        sel = list(range(6)) if states is None else sorted(set(int(j) for j in states))
        if any(j < 0 or j >= 32 for j in sel):
            raise Exception("start_log: states must be indices of the vessel's state (nedx, nedy, psi, u, v, r)")
        d.state_mask = sum(1 << j for j in sel)
        d.record_thrust, d.record_ref, d.record_err, d.record_status = (int(bool(v)) for v in (thrust, ref, err, status))
        ptrs = [C.c_void_p(self.ll.device_ptr(f)) for f in ("status", "qp_iter")] if status else [None, None]
        self._check(self._lib.usvmpc_cascade_log_start(self._c, C.byref(d), *ptrs))
        self._log = dict(states=sel, first=d.first, every=d.every, thrust=bool(thrust), ref=bool(ref), err=bool(err), status=bool(status))

    def log_info(self):
        """dict: records made, ticks counted since start_log, missed (due for a record when the buffer was full), nsel."""
        r, n = C.c_int(), C.c_int()
        tk, mi = C.c_longlong(), C.c_longlong()
        self._check(self._lib.usvmpc_cascade_log_info(self._c, C.byref(r), C.byref(tk), C.byref(mi), C.byref(n)))
        return dict(records=r.value, ticks=tk.value, missed=mi.value, nsel=n.value)

    def read_log(self, records=None, instances=None):
        """The log so far (synchronises).  records / instances: None (all made so far / the batch) or a half-open (start, stop) pair or range.
        dict: state [nb][nrec][nsel], thrust, ref [nb][nrec][2] (float64), err [nb][nrec][2] (float32) - instance-major views of the
        tick-major copy -, ll_status, ll_qp_iter, g_status, g_qp_iter [nb][nrec] (the status word, unpacked), tick [nrec] (the tick of each
        record), states (the indices of state's last axis).  Channels not recorded are absent."""
        made = self.log_info()["records"]    # (raises when no log runs)
        lg = self._log
        rng = self.ll._log_range
        r0, nr = rng(records, made, "records")
        b0, nb = rng(instances, self.B, "instances")
        out = dict(tick=lg["first"] + lg["every"] * np.arange(r0, r0 + nr), states=list(lg["states"]))
        chans = [("state", len(lg["states"]), np.float64)] if lg["states"] else []
        chans += [(name, 2, dt) for name, dt in (("thrust", np.float64), ("ref", np.float64), ("err", np.float32)) if lg[name]]
        chans += [("status", 1, np.int32)] if lg["status"] else []
        for name, n, dt in chans:
            a = np.zeros((nr, nb, n), dtype=dt)
            if nr > 0 or records is not None:
                self._check(self._lib.usvmpc_cascade_log_read(self._c, name.encode(), r0, nr, b0, nb, a.ctypes.data_as(C.c_void_p), a.nbytes))
            if name == "status":
                w = a[:, :, 0].T
                out["ll_status"], out["ll_qp_iter"] = w & 0xff, (w >> 8) & 0xff
                out["g_status"], out["g_qp_iter"] = (w >> 16) & 0xff, (w >> 24) & 0x7f
            else:
                out[name] = a.transpose(1, 0, 2)
        return out

    def log_device_ptr(self, channel):
        """Device address of a log channel ("state", "thrust", "ref", "err", "status") for zero-copy views."""
        p = C.c_void_p()
        self._check(self._lib.usvmpc_cascade_log_device_ptr(self._c, channel.encode(), C.byref(p)))
        return p.value

    def stop_log(self):
        self._check(self._lib.usvmpc_cascade_log_stop(self._c))
        self._log = None

    # -- the realised cost of both layers (include/usvmpc.h, "Objective value": usvmpc_cost_track_now)
    def track_cost(self, on=True):
        """While on, tick() adds c_0(x0, u_0, yref_0, sl_0, su_0) of the guidance layer to its tracked sum right after every guidance solve,
        and that of the low level right after every low-level solve, ahead of the step.  on=True (again) zeroes sums and counts; on=False
        stops and frees.  (A hand-written loop calls g.track_cost_now() / ll.track_cost_now() at the same places.)"""
        self.g.track_cost(on)
        self.ll.track_cost(on)
        self._track = bool(on)

    def tracked_cost(self):
        """dict(guidance=(sum [B], count), low_level=(sum [B], count)); synchronises."""
        return dict(guidance=self.g.tracked_cost(), low_level=self.ll.tracked_cost())

    def close(self):
        """before either solver is closed"""
        if self._c is not None:
            if self._log is not None:
                self._lib.usvmpc_cascade_log_stop(self._c)
                self._log = None
            self._lib.usvmpc_cascade_destroy(self._c)
            self._c = None
