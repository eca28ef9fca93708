"""numpy restatement of the path-following node's front end (catkin_ws/src/nmpc_ca/src/nmpc_pf.cpp: velocityCallback :198-206,
waypoint_manager :226-268, control :270-377, main :392-401), one instance at a time, written from those lines - not from
csrc/pf_guidance.hpp, which the tests compare against it.  The obstacle side (the node has none) follows the issue's statement: selection in
the NED frame by distance - (R + 0.5), strict visibility test, lh = (R + 0.5) + margin.

Like the node, PfRef rewrites yref on EVERY active tick; `yref_writes` counts what the device's rule would write (triple changed bit for bit,
or stale), so that equal yref arrays show the rule loses nothing."""
import numpy as np

OVER, ACTIVE, SWITCH = 0, 1, 2
BOAT_RADIUS = 0.5


def select(world, K, nedx, nedy, max_radius, margin):
    """-> p [2K], lh [K], chosen [K] (-1: parked), smallest d over the visible ones (1e300: none)"""
    p, lh, chosen = np.full(2 * K, 1000.0), np.zeros(K), np.full(K, -1, dtype=int)
    world = np.asarray(world, dtype=float).reshape(-1, 3)
    if len(world) == 0:
        return p, lh, chosen, 1e300
    dx, dy = world[:, 0] - nedx, world[:, 1] - nedy
    dist = np.sqrt(dx * dx + dy * dy)
    d = dist - (world[:, 2] + BOAT_RADIUS)
    vis = np.nonzero(dist < max_radius)[0]
    if len(vis) == 0:
        return p, lh, chosen, 1e300
    order = vis[np.argsort(d[vis], kind="stable")]          # ascending, ties by list index
    for slot, i in enumerate(order[:K]):
        p[2 * slot], p[2 * slot + 1] = world[i, 0], world[i, 1]
        lh[slot] = (world[i, 2] + BOAT_RADIUS) + margin
        chosen[slot] = i
    return p, lh, chosen, float(d[vis].min())


class PfRef:
    def __init__(self, B, N, K, margin=0.2):
        self.B, self.N, self.K, self.margin = B, N, K, margin
        self.x0 = np.zeros((B, 14))
        self.yref = np.zeros((B, N, 16))
        self.yref_e = np.zeros((B, 14))
        self.p0 = np.zeros((B, 2 * K))
        self.lh0 = np.zeros((B, K))
        self.world = np.zeros((B, 0, 3))
        self.max_radius = 100.0

    def reset(self, waypoints):
        B = self.B
        w = np.asarray(waypoints, dtype=float)
        self.wp = np.tile(w[None], (B, 1, 1)) if w.ndim == 2 else w.reshape(B, -1, 2)
        self.npts = self.wp.shape[1]
        self.k = np.ones(B, dtype=int)                        # :394
        self.phase = np.full(B, SWITCH)
        self.finish_tick = np.full(B, -1)
        self.past = np.zeros((B, 2))                          # :172-173
        self.last = np.full((B, 3), np.nan)
        self.u, self.ye = np.zeros(B), np.zeros(B)
        self.min_clearance = np.full(B, 1e300)
        self.chosen = np.full((B, self.K), -1)
        self.yref_writes = 0
        self.stale = True
        self.tick = 0
        self.out = dict(thr_port=np.zeros(B), thr_stbd=np.zeros(B), Tx=np.zeros(B), Tz=np.zeros(B), speed=np.zeros(B),
                        e_u=np.zeros(B, dtype=np.float32), e_ye=np.zeros(B, dtype=np.float32), active=np.zeros(B, dtype=np.int32))

    def set_world(self, world, max_radius=100.0):
        w = np.asarray(world, dtype=float)
        self.world = np.tile(w[None], (self.B, 1, 1)) if w.ndim == 2 else w.reshape(self.B, -1, 3)
        self.max_radius = max_radius

    def prepare(self, vel=None, pose=None):
        """vel, pose None: device-resident (reads self.x0)."""
        self.wrote = np.zeros(self.B, dtype=bool)
        for b in range(self.B):
            if vel is None:
                x = self.x0[b]
                u, v, r, psi, nedx, nedy, pp, ps = x[3], x[4], x[5], x[0], x[10], x[11], x[12], x[13]
            else:
                (u, v, r), (nedx, nedy, psi) = vel[b], pose[b]
                pp, ps = self.past[b]
            if u == 0:                                        # :201-203
                u = 0.001
            k = self.k[b]
            if k < self.npts:                                 # :228
                x1, y1 = self.wp[b, k - 1]
                x2, y2 = self.wp[b, k]
                dx, dy = x2 - nedx, y2 - nedy
                distance = np.sqrt(dx * dx + dy * dy)         # :237-239
                u_des = 0.7
                if distance > 1:                              # :243
                    ak = np.arctan2(y2 - y1, x2 - x1)
                    sa, ca = np.sin(ak), np.cos(ak)
                    ye = -(nedx - x1) * sa + (nedy - y1) * ca
                    phase = ACTIVE
                else:
                    self.k[b] = k + 1                         # :255
                    phase = SWITCH
            else:
                phase = OVER
                if self.finish_tick[b] < 0:
                    self.finish_tick[b] = self.tick
            self.phase[b] = phase
            if phase != OVER:
                self.p0[b], self.lh0[b], self.chosen[b], dmin = select(self.world[b], self.K, nedx, nedy, self.max_radius, self.margin)
                self.min_clearance[b] = min(self.min_clearance[b], dmin)
            if phase == ACTIVE:
                beta = np.arctan2(v, u + .001)                # :273
                chi = psi + beta
                self.x0[b] = [psi, np.sin(chi), np.cos(chi), u, v, r, ye, x1, y1, ak, nedx, nedy, pp, ps]   # :278-291
                yr = np.zeros(16)
                yr[1], yr[2], yr[3] = sa, ca, u_des           # :299-314
                self.yref[b] = yr
                self.yref_e[b] = yr[:14]
                self.u[b], self.ye[b] = u, ye
                triple = np.array([sa, ca, u_des])
                if self.stale or triple.tobytes() != self.last[b].tobytes():
                    self.yref_writes += 1
                    self.wrote[b] = True
                    self.last[b] = triple
            elif self.stale:
                self.last[b] = np.nan
        self.stale = False
        self.tick += 1

    def publish(self, x1_state):
        """x1_state [B, 14]: stage 1 of the solve."""
        o = self.out
        for b in range(self.B):
            ph = self.phase[b]
            o["active"][b] = 1 if ph == ACTIVE else 0
            if ph == ACTIVE:
                port, stbd = x1_state[b, 12], x1_state[b, 13]   # :349-350
                o["thr_port"][b], o["thr_stbd"][b] = port, stbd
                self.past[b] = port, stbd                       # :359-360
                o["e_u"][b] = np.float32(0.7 - self.u[b])       # :362
                o["e_ye"][b] = np.float32(0.0 - self.ye[b])     # :363
                o["Tx"][b] = port + 0.78 * stbd                 # :372
                o["Tz"][b] = (port - 0.78 * stbd) * 0.41 / 2    # :373
                o["speed"][b] = 0.7
            elif ph == OVER:                                    # :260-266
                o["thr_port"][b] = o["thr_stbd"][b] = o["speed"][b] = 0.0
        return {k: v.copy() for k, v in o.items()}


def scripted_sequence(B, ticks, seed=5, classes=None):
    """Waypoints (npts = 3), and per tick vel [B,3] / pose [B,3] that cover: an ordinary tick; u == 0; a switch tick (nothing written, k
    advanced); the tick after it (new segment); mission end; distance exactly 1 (waypoint (0, 0), pose (1, 0)).  Poses otherwise keep
    1e-9 clear of the switch radius.  Instance classes by b % 6:
      0 cruises along leg 1;  1 has u == 0 on tick 1;  2 reaches waypoint 1 at tick 3 (switch), then follows leg 2;
      3 starts on leg 2's end region: switches at tick 2 -> mission over from tick 3;  4 sits at distance exactly 1 of ITS waypoint 1 = (0, 0)
      on tick 4;  5 cruises with a sway.  classes: the class of each instance instead of b % 6."""
    rng = np.random.default_rng(seed)
    wps = np.tile(np.array([[4.0, -5.0], [4.0, 1.0], [8.0, 5.0]])[None], (B, 1, 1))
    cls = np.arange(B) % 6 if classes is None else np.asarray(classes, dtype=int)
    wps[cls == 4] = np.array([[-6.0, 0.0], [0.0, 0.0], [3.0, 4.0]])
    vel = np.zeros((ticks, B, 3))
    pose = np.zeros((ticks, B, 3))
    jx = rng.uniform(-0.8, 0.8, B)
    for t in range(ticks):
        vel[t, :, 0] = 0.5 + 0.02 * t + rng.uniform(0.0, 0.2, B)
        vel[t, :, 1] = np.where(cls == 5, rng.uniform(-0.1, 0.1, B), 0.0)
        vel[t, :, 2] = rng.uniform(-0.05, 0.05, B)
        pose[t, :, 0] = 4.0 + jx
        pose[t, :, 1] = -4.5 + 0.03 * t
        pose[t, :, 2] = np.pi / 2 + rng.uniform(-0.2, 0.2, B)
        m = cls == 1
        if t == 1:
            vel[t, m, 0] = 0.0
        m = cls == 2                                            # approaches (4, 1): inside 1 m at tick 3, then on leg 2
        pose[t, m, 0] = 4.0 + 0.1 * jx[m]
        pose[t, m, 1] = [-1.5, -0.8, -0.2, 0.3, 0.6, 0.9][min(t, 5)] + (0.05 * (t - 5) if t > 5 else 0.0)
        m = cls == 3                                            # near (4, 1) at once (switch at tick 0), near (8, 5) at tick 2 (switch) -> over
        pose[t, m, 0] = [4.1, 6.0, 7.8][min(t, 2)]
        pose[t, m, 1] = [0.8, 3.0, 4.7][min(t, 2)]
        m = cls == 4
        pose[t, m, 0] = -3.1 + 0.4 * t
        pose[t, m, 1] = 0.02 * jx[m]
        if t == 4:
            pose[t, m, 0], pose[t, m, 1] = 1.0, 0.0             # distance to (0, 0) exactly 1: switches (the node tests distance > 1)
    # keep clear of the switch radius elsewhere
    for t in range(ticks):
        for k in (1, 2):
            d = np.hypot(wps[:, k, 0] - pose[t, :, 0], wps[:, k, 1] - pose[t, :, 1])
            near = np.abs(d - 1.0) < 1e-9
            near &= ~((cls == 4) & (t == 4))
            assert not near.any()
    return wps, vel, pose


EXACT_X0 = [0, 3, 4, 5, 7, 8, 10, 11, 12, 13]      # psi, u, v, r, x1, y1, nedx, nedy, past thrust: no transcendental enters
TRIG_X0 = [1, 2, 6, 9]                             # sin chi, cos chi, ye, ak
TOL = 1e-12                                        # values that pass through sin / cos / atan2 (tests/test_guidance.py uses it for M1's x0)


def check(ref, got, what=""):
    """got: dict with any of k, phase / active, finish_tick, x0, yref, yref_e, p0, lh0, min_clearance, out (publish dict) - against PfRef
    under the issue's rules: exact wherever no transcendental enters, 1e-12 absolute otherwise."""
    def same(a, b, name):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), "%s %s:\n%r\n%r" % (what, name, a, b)

    def close(a, b, name):
        err = np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float)).max() if np.size(a) else 0.0
        assert err <= TOL, "%s %s: %.3g" % (what, name, err)
    if "k" in got:
        same(got["k"], ref.k, "k")
    if "phase" in got:
        same(got["phase"], ref.phase, "phase")
    if "finish_tick" in got:
        same(got["finish_tick"], ref.finish_tick, "finish_tick")
    if "x0" in got:
        same(got["x0"][:, EXACT_X0], ref.x0[:, EXACT_X0], "x0 (exact columns)")
        close(got["x0"][:, TRIG_X0], ref.x0[:, TRIG_X0], "x0 (sin chi, cos chi, ye, ak)")
    if "yref" in got:
        close(got["yref"], ref.yref, "yref")
        same(np.delete(got["yref"], [1, 2], axis=2), np.delete(ref.yref, [1, 2], axis=2), "yref (u_des and zeros)")
    if "yref_e" in got:
        close(got["yref_e"], ref.yref_e, "yref_e")
    if "p0" in got:
        same(got["p0"], ref.p0, "p stage 0")
    if "lh0" in got:
        same(got["lh0"], ref.lh0, "lh stage 0")
    if "min_clearance" in got:
        same(got["min_clearance"], ref.min_clearance, "min_clearance")
    if "out" in got:
        o, r = got["out"], ref.out
        for nm in ("thr_port", "thr_stbd", "Tx", "Tz", "speed", "e_u", "active"):
            same(o[nm], r[nm], nm)
        close(o["e_ye"], r["e_ye"], "e_ye")
