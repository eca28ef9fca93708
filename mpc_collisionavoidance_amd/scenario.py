"""Synthetic batch workloads: LiDAR obstacle-scenario sweeps about the
reference's path-following scenario.

Inputs are derived the way the reference's callers derive them (paths relative to
/root/reference/catkin_ws/src/nmpc_ca/): cross-track error and course error as
src/nmpc_guidance_ca1.cpp:460-461,495-511; the pf_ca state and yref as
scripts/usv_pf_ca/main.py:95-133; obstacle radius = R + boat radius 0.5
(src/nmpc_guidance_ca1.cpp:139,319), lh = R (soft model, +0.2 through lsh) or R + 0.2 (hard model,
scripts/usv_pf_ca/main.py:126); unused slots at (1000,1000) with r = 0
(src/nmpc_guidance_ca1.cpp:365-376).  Pure numpy; no solver code here.
"""
import numpy as np

PATH = (4.0, -5.0, 4.0, 25.0)  # (x1, y1) -> (x2, y2), scripts/usv_guidance_ca1/main.py:99-102


def wrap(a):
    return (a + np.pi) % (2.0 * np.pi) - np.pi


# Shooting interval per model.  usv_model / usv_model_guidance_ca1: 0.05 s as the reference
# (scripts/usv_acados/main.py:52-53, scripts/usv_guidance_ca1/main.py:54-55).  usv_model_pf_ca:
# 0.01 s as the reference (scripts/usv_pf_ca/main.py:54-55) - its sway damping Yv = -19890|v| is
# stiff and the explicit RK4 map is unstable at 0.05 s once |v| > 0.07.
DT = {"usv_model": 0.05, "usv_model_guidance_ca1": 0.05, "usv_model_pf_ca": 0.01}

# Benchmark settings: shooting interval 0.05 s for EVERY model, i.e. Tf = 2 s at N = 40.
# usv_model_pf_ca cannot take one RK4 step of 0.05 s (see above), so its integrator runs 5 steps per interval
# (acados sim_method_num_steps = 5): the integration step stays the reference's 0.01 s while the look-ahead is
# the 2 s the obstacle rows need to become active.  NOISE_MASK: states the closed-loop disturbance is added to -
# every state for the soft-row model, (u, r) for usv_model_pf_ca as the reference's own "Add noise" hooks have it
# (scripts/usv_pf_ca/main.py:181-183: x0[3], x0[5]; position noise on a vehicle that grazes a HARD keep-out
# circle makes the next QP infeasible by construction).
BENCH_DT = 0.05
BENCH_SIM_STEPS = {"usv_model": 1, "usv_model_guidance_ca1": 1, "usv_model_pf_ca": 5}
NOISE_MASK = {"usv_model": (1 << 5) - 1, "usv_model_guidance_ca1": (1 << 8) - 1, "usv_model_pf_ca": (1 << 3) | (1 << 5)}

ALL_STATES_MASK = (1 << 14) - 1   # SURVEY.md 8(d) as worded: "x0 <- previous x1 + N(0, 1e-3)" on every state

_CY = 0.5 * (-40.0 * 1000.0) * (1.1 + 0.0045 * (1.01 / 0.09) - 0.1 * (0.27 / 0.09) + 0.016 * ((0.27 / 0.09) ** 2))


def _pf_ca_rhs(y, ak, Tp, Ts):
    """usv_model_pf_ca right-hand side with zero input (thrusts constant), vectorised over the batch
    (scripts/usv_pf_ca/usv_model.py:137-160).  y = rows (psi, sinpsi, cospsi, u, v, r, ye, nedx, nedy) of shape [9, B]:
    the states that move; only used to roll the initial guess forward."""
    m, Iz, Bw = 30.0, 4.1, 0.41
    Xud, Yvd, Yrd, Nvd, Nrd = -2.25, -23.13, -1.31, -16.41, -2.79
    Yvv, Yvr, Nrv, Nrr = -99.99, -5.49, -8.8, -3.49
    psi, u, v, r = y[0], y[3], y[4], y[5]
    fast = u > 1.25
    Xu, Xuu = np.where(fast, 64.55, -25.0), np.where(fast, -70.92, 0.0)
    au, av, ar = np.abs(u), np.abs(v), np.abs(r)
    Nr = -0.52 * np.sqrt(u * u + v * v)
    a = Yrd + Nvd
    f = np.empty_like(y)
    chi = psi + np.arctan2(v, u + 0.001)
    sp, cp = np.sin(psi), np.cos(psi)
    vx, vy = u * cp - v * sp, u * sp + v * cp
    f[0] = r
    f[1] = np.cos(chi) * r
    f[2] = -np.sin(chi) * r
    f[3] = ((Tp + Ts) - (-m + 2.0 * Yvd) * v - a * r * r - (-Xu * u - Xuu * au * u)) / (m - Xud)
    f[4] = (-(m - Xud) * u * r - (-_CY * av - Yvv * av - Yvr * ar) * v) / (m - Yvd)
    f[5] = ((Tp - Ts) * (Bw / 2.0) - (-2.0 * Yvd * u * v - a * r * u + Xud * u * r) -
            (-Nr * r - Nrv * av * r - Nrr * ar * r)) / (Iz - Nrd)
    f[6] = -vx * np.sin(ak) + vy * np.cos(ak)
    f[7] = vx
    f[8] = vy
    return f


def _pf_ca_rollout(x0, N, dt, steps):
    """Zero-input simulation with the solver's own integrator (RK4, `steps` steps per interval): [B, N+1, nx]."""
    h = dt / steps
    mov = [0, 1, 2, 3, 4, 5, 6, 10, 11]
    y = np.ascontiguousarray(x0[:, mov].T)
    ak, Tp, Ts = x0[:, 9].copy(), x0[:, 12].copy(), x0[:, 13].copy()
    out = np.repeat(x0[:, None, :], N + 1, axis=1)
    for k in range(N):
        for _ in range(steps):
            k1 = _pf_ca_rhs(y, ak, Tp, Ts)
            k2 = _pf_ca_rhs(y + 0.5 * h * k1, ak, Tp, Ts)
            k3 = _pf_ca_rhs(y + 0.5 * h * k2, ak, Tp, Ts)
            k4 = _pf_ca_rhs(y + h * k3, ak, Tp, Ts)
            y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        out[:, k + 1, mov] = y.T
    return out


def make_batch(name, N, K, B, dt=None, seed=1234, moving=False, n_active=None, generator="beside", sim_steps=1,
               max_range=6.0, clip_time=1.2):
    """Returns dict(x0 [B,nx], yref [B,N,ny], yref_e [B,nx], p [B,N+1,2K], lh [B,N,K],
    x_init [B,N+1,nx], u_init [B,N,nu]).

    generator (obstacle placement and initial guess of usv_model_pf_ca; the other models have one):
      "survey" - SURVEY.md 8(d): sway v ~ U(-0.1, 0.1); obstacles in polar form about the vehicle (bearing within
                 +-60 deg of the course, range R+0.7 .. 6 m), with ONE stated clip: an obstacle whose keep-out circle
                 the course ray would enter closer than 0.4 m + 1.2 s * u is moved outwards along its bearing until it
                 does not (hard rows: nearer than that the first QP has no feasible point - the vehicle can neither
                 stop nor turn in time); initial guess = zero-input simulation with the solver's integrator.
      "survey_verbatim" - SURVEY.md 8(d) to the letter: the same draws as "survey" (same seed -> same vehicles, same obstacles before
                 the clip), NO clip, and acados' own initial guess x_k = x0, u = 0.  For usv_model_pf_ca's hard rows that means a
                 share of first QPs without a feasible point (the line reports them: status_nonzero_frac, qp_not_converged_frac).
      "beside" - round-1 workload for the reference's dt = 0.01 s (0.4 s look-ahead at N = 40): v ~ U(-0.03, 0.03),
                 obstacles beside the straight-line roll-out; kept for the parity tests at the reference's step size."""
    if dt is None:
        dt = DT[name]
    if generator not in ("survey", "survey_verbatim", "beside"):
        raise ValueError(generator)
    verbatim = generator == "survey_verbatim"
    survey = generator in ("survey", "survey_verbatim") and name == "usv_model_pf_ca"
    rng = np.random.default_rng(seed)
    x1, y1, x2, y2 = PATH
    ak = np.arctan2(y2 - y1, x2 - x1)
    nedx = rng.uniform(2.0, 6.0, B)
    nedy = rng.uniform(-5.0, 15.0, B)
    psi = ak + rng.uniform(-0.6, 0.6, B)
    u = rng.uniform(0.3, 1.2, B)
    v = rng.uniform(-0.1, 0.1, B) if (name == "usv_model_guidance_ca1" or survey) else rng.uniform(-0.03, 0.03, B)
    r = rng.uniform(-0.1, 0.1, B)
    Tp = rng.uniform(0.0, 15.0, B)
    Ts = rng.uniform(0.0, 15.0, B)
    ye = -(nedx - x1) * np.sin(ak) + (nedy - y1) * np.cos(ak)
    beta = np.arctan2(v, u + 0.001)
    course = psi + beta
    if name == "usv_model":
        nx, nu = 5, 2
        x0 = np.stack([u, v, r, Tp, Ts], axis=1)
        yr = np.zeros(nx + nu)
        yr[0] = 1.3  # scripts/usv_acados/main.py:73
        yref = np.tile(yr, (B, N, 1))
        yref_e = np.tile(yr[:nx], (B, 1))
    elif name == "usv_model_guidance_ca1":
        nx, nu = 8, 1
        chie = wrap(psi + beta - ak)
        psied = wrap(psi - ak)
        x0 = np.stack([u, v, ye, chie, psied, nedx, nedy, psi], axis=1)
        yref = np.zeros((B, N, nx + nu))
        yref_e = np.zeros((B, nx))
    elif name == "usv_model_pf_ca":
        nx, nu = 14, 2
        x0 = np.stack([psi, np.sin(psi), np.cos(psi), u, v, r, ye, np.full(B, x1), np.full(B, y1),
                       np.full(B, ak), nedx, nedy, Tp, Ts], axis=1)
        yr = np.zeros(nx + nu)
        yr[1], yr[2], yr[3] = np.sin(ak), np.cos(ak), 0.7
        yref = np.tile(yr, (B, N, 1))
        yref_e = np.tile(yr[:nx], (B, 1))
    else:
        raise ValueError(name)
    K = int(K)
    p = np.zeros((B, N + 1, 2 * K))
    lh = np.zeros((B, N, K))
    obs_pos, obs_vel = np.zeros((B, K, 2)), np.zeros((B, K, 2))
    if K:
        na = K if n_active is None else int(n_active)
        R = rng.uniform(0.3, 1.5, (B, K)) + 0.5
        margin = 0.0 if name == "usv_model_guidance_ca1" else 0.2
        lhv = R + margin
        if name == "usv_model_guidance_ca1" or survey:
            # polar about the vehicle: bearing within +-60 deg of the course, range R+0.7 .. 6 m
            rad = (R + 0.7) + rng.uniform(0.0, 1.0, (B, K)) * np.maximum(max_range - (R + 0.7), 0.0)
            rel = rng.uniform(-np.pi / 3, np.pi / 3, (B, K))
            if survey and not verbatim:
                # hard rows: the course ray enters the keep-out circle (radius lh) at s = lon - sqrt(lh^2 - lat^2);
                # obstacles with s < s_min(u) move out along their bearing to the range where s = s_min
                smin = (0.4 + clip_time * u)[:, None]
                lat, lon = rad * np.sin(rel), rad * np.cos(rel)
                hit = np.abs(lat) < lhv
                s_enter = np.where(hit, lon - np.sqrt(np.maximum(lhv ** 2 - lat ** 2, 0.0)), np.inf)
                cb = np.cos(rel)
                # s_enter grows with the range; it equals s_min at the larger root of the quadratic below PROVIDED that
                # root still has the centre beyond s_min (lon >= s_min) - otherwise the chord the ray cuts vanishes
                # first, and the obstacle moves out to where the ray is tangent to its circle
                disc = (smin * cb) ** 2 - (smin ** 2 - lhv ** 2)
                root = smin * cb + np.sqrt(np.maximum(disc, 0.0))
                tangent = lhv / np.maximum(np.abs(np.sin(rel)), 1e-12)
                rad_out = np.where((disc >= 0.0) & (root * cb >= smin), root, tangent)
                rad = np.where(hit & (s_enter < smin), np.maximum(rad, rad_out) + 1e-9, rad)
            bearing = course[:, None] + rel
            ox = nedx[:, None] + rad * np.cos(bearing)
            oy = nedy[:, None] + rad * np.sin(bearing)
        else:
            # hard rows, short look-ahead L = u*N*dt: obstacles beside the straight-line prediction,
            # keep-out circle 0.01 .. 0.51 m clear of it (quadratic skew towards grazing), abeam of a point 0 .. 1.5 L ahead
            L = (u * N * dt)[:, None]
            s_al = rng.uniform(0.0, 1.5, (B, K)) * L
            clear = 0.01 + 0.5 * rng.uniform(0.0, 1.0, (B, K)) ** 2
            side = np.where(rng.uniform(0.0, 1.0, (B, K)) < 0.5, -1.0, 1.0)
            cx_, cy_ = np.cos(course)[:, None], np.sin(course)[:, None]
            off = side * (lhv + clear)
            ox = nedx[:, None] + s_al * cx_ - off * cy_
            oy = nedy[:, None] + s_al * cy_ + off * cx_
        if na < K:
            ox[:, na:], oy[:, na:], lhv[:, na:] = 1000.0, 1000.0, 0.0
        if not moving:
            vel = np.zeros((B, K, 2))
        elif name == "usv_model_guidance_ca1" or survey:
            vel = rng.uniform(-0.3, 0.3, (B, K, 2))
            if survey:
                # hard rows: an obstacle that closes in on the vehicle cannot be answered by a slack; the component of its
                # velocity towards the vehicle's position is removed (it may still cross the path ahead)
                er = np.stack([ox - nedx[:, None], oy - nedy[:, None]], axis=2)
                er /= np.linalg.norm(er, axis=2, keepdims=True)
                vr = (vel * er).sum(axis=2, keepdims=True)
                vel = vel - np.minimum(vr, 0.0) * er
        else:
            # hard rows: obstacles slide parallel to the course, which keeps their lateral clearance
            # (a drift towards the path would make the hard-constrained QPs infeasible)
            vpar = rng.uniform(-0.3, 0.3, (B, K))
            vel = np.stack([vpar * np.cos(course)[:, None], vpar * np.sin(course)[:, None]], axis=2)
        t = (np.arange(N + 1) * dt)[None, :, None]
        p[:, :, 0::2] = ox[:, None, :] + t * vel[:, None, :, 0]
        p[:, :, 1::2] = oy[:, None, :] + t * vel[:, None, :, 1]
        lh[:] = lhv[:, None, :]
        obs_pos, obs_vel = np.stack([ox, oy], axis=2), np.ascontiguousarray(vel)   # the tracks p was made from (predict_tracks)
    # initial guess: kinematic straight-line rollout (constant body velocities, u = 0).  acados'
    # own cold start x_k = x0 linearises every stage's obstacle rows at the current position,
    # which makes the hard rows of usv_model_pf_ca mutually inconsistent with moving at all.
    x_init = np.tile(x0[:, None, :], (1, N + 1, 1))
    tk = (np.arange(N + 1) * dt)[None, :]
    vx = (u * np.cos(psi) - v * np.sin(psi))[:, None]
    vy = (u * np.sin(psi) + v * np.cos(psi))[:, None]
    yed = -vx * np.sin(ak) + vy * np.cos(ak)
    if verbatim:
        pass  # x_k = x0: what AcadosOcpSolver starts from when the caller sets nothing (scripts/usv_pf_ca/main.py sets no iterate)
    elif name == "usv_model_guidance_ca1":
        x_init[:, :, 2] += tk * yed
        x_init[:, :, 5] += tk * vx
        x_init[:, :, 6] += tk * vy
    elif survey:
        x_init = _pf_ca_rollout(x0, N, dt, sim_steps)
    elif name == "usv_model_pf_ca":
        x_init[:, :, 6] += tk * yed
        x_init[:, :, 10] += tk * vx
        x_init[:, :, 11] += tk * vy
    u_init = np.zeros((B, N, nu))
    return dict(x0=x0, yref=yref, yref_e=yref_e, p=p, lh=lh, x_init=x_init, u_init=u_init,
                nx=nx, nu=nu, K=K, N=N, dt=dt, sim_steps=sim_steps, generator=generator,
                obs_pos=obs_pos, obs_vel=obs_vel)


def predict_tracks(pos, vel, N, dt):
    """p [B, N+1, 2K] of obstacle tracks pos, vel [B, K, 2]: stage k holds pos + (k dt) vel - the expression make_batch builds p with, so
    predict_tracks(wl["obs_pos"], wl["obs_vel"], N, dt) IS wl["p"], bit for bit, and so is what the device derives under option
    "obstacle_tracks" (csrc/obstacle_tracks.hpp: product and sum rounded separately)."""
    pos, vel = np.asarray(pos, dtype=float), np.asarray(vel, dtype=float)
    B, K = pos.shape[0], pos.shape[1]
    p = np.zeros((B, N + 1, 2 * K))
    t = (np.arange(N + 1) * dt)[None, :, None]
    p[:, :, 0::2] = pos[:, None, :, 0] + t * vel[:, None, :, 0]
    p[:, :, 1::2] = pos[:, None, :, 1] + t * vel[:, None, :, 1]
    return p


def make_bench_batch(name, N, K, B, seed=1234, moving=False, verbatim=False, n_active=None):
    """The benchmark workload of SURVEY.md 8(d) for `name`: dt = 0.05 s, the "survey" generator.  SURVEY's obstacle field
    (range up to 6 m, course ray clear for 0.4 m + 1.2 s * u) is sized for the 2 s look-ahead of N = 40; other horizons scale
    both with it.  Shorter (BASELINE configs[1], Tf = 1 s): range up to 3 Tf metres, clear for 0.6 Tf - with the 2 s field a 1 s
    look-ahead never reaches an obstacle (2 % of the instances with an active row after 12 closed-loop ticks; scaled: 71 %, no
    failed solve).  Longer (configs[4], Tf = 4 s): range up to 3 Tf, clear for 1.1 Tf - at N = 80 the same circles in the same
    6 m sector wall the vehicle in and a third of the hard-row QPs have no feasible point.
    verbatim: SURVEY.md 8(d) without the builder's departures (make_batch, "survey_verbatim"): no obstacle clip, x_k = x0 as the initial
    guess; the disturbance then goes on every state (ALL_STATES_MASK); the 5 RK4 steps of usv_model_pf_ca stay - one RK4 step of 0.05 s
    is outside the model's stability region (DT above), the solves would be NaN."""
    Tf = N * BENCH_DT
    long_h = Tf > 2.0 + 1e-9
    return make_batch(name, N, K, B, dt=BENCH_DT, seed=seed, moving=moving, generator="survey_verbatim" if verbatim else "survey",
                      n_active=n_active,   # (fewer obstacles than slots: the rest parked at (1000, 1000), r = 0 - nmpc_guidance_ca1.cpp:365-376)
                      sim_steps=BENCH_SIM_STEPS[name], max_range=3.0 * Tf,
                      clip_time=1.1 * Tf if long_h else 0.6 * Tf)


def load_into(solver, wl):
    """Push a workload into a BatchOcpSolver (iterate initialised to x_k = x0, u = 0)."""
    solver.set("x0", 0, wl["x0"])
    solver.set_all("x", wl["x_init"])
    solver.set_all("u", wl["u_init"])
    solver.set_all("yref", wl["yref"])
    solver.set("yref", solver.N, wl["yref_e"])
    if wl["K"]:
        solver.set_all("p", wl["p"])
        solver.set_all("lh", wl["lh"])


def load_tracks(solver, wl):
    """Hand a workload's obstacle tracks to a BatchOcpSolver and switch it to deriving p from them (after load_into: lh stays the
    caller's).  From then on solver.advance / advance_sim move the obstacles along with the vehicle."""
    if wl["K"]:
        solver.set_obstacle_tracks(wl["obs_pos"], wl["obs_vel"])


# ---- Path-following missions for usv_model_pf_ca behind guidance.PathFollowingFrontEnd: two legs, four obstacles beside them.
PF_MISSION_WAYPOINTS = np.array([[4.0, -5.0], [4.0, 1.0], [8.0, 5.0]])
PF_MISSION_OCP = dict(N=40, dt=0.05, sim_steps=5, K=4, max_radius=100.0, margin=0.2)


# moving=True: obstacle i drifts at a constant velocity, U(-PF_DRIFT_ALONG, PF_DRIFT_ALONG) m/s along its own leg and
# U(-PF_DRIFT_ACROSS, PF_DRIFT_ACROSS) m/s along the leg's normal (the vessel cruises at 0.7 m/s).  Settled with tools/pf_mission_oracle.py.
PF_DRIFT_ALONG, PF_DRIFT_ACROSS = 0.15, 0.05


def make_pf_missions(B, seed=0, moving=False):
    """B missions, instance b drawn from numpy.random.default_rng(seed + b) - an instance does not depend on the batch it is in.
    Returns dict(waypoints [B,3,2], world [B,4,3] = (X, Y, R), x0 [B,14]).  Obstacle i lies beside leg i % 2: a point t ~ U(0.25, 0.8)
    along the leg, moved 0.9 .. 1.6 m along the leg's unit normal (-dy, dx) / |.| to either side, radius 0.1 .. 0.4 m (keep-out radius
    R + 0.5 + 0.2: the path stays free by 0.1 m at least, the vessel has to swerve for the nearer ones).  Nearer obstacles (0.5 .. 0.9 m)
    leave a third of the missions stuck in front of a hard row: this spacing is deliberate.  The vessel starts at (4 +- 1, -5), heading
    pi/2 +- 0.3, u = 0.001, everything else 0.
    moving=True adds world_vel [B,4,2] (vX, vY), drawn from a stream of its own, default_rng([seed + b, 1]): every other field is the
    same bits with either value of `moving`."""
    w = PF_MISSION_WAYPOINTS
    world = np.zeros((B, 4, 3))
    x0 = np.zeros((B, 14))
    vel = np.zeros((B, 4, 2))
    for b in range(B):
        rng = np.random.default_rng(seed + b)
        for i in range(4):
            leg = i % 2
            t = rng.uniform(0.25, 0.8)
            d = w[leg + 1] - w[leg]
            c = w[leg] + t * d
            n = np.array([-d[1], d[0]]) / np.hypot(d[0], d[1])
            off = rng.uniform(0.9, 1.6)
            sign = 1.0 if rng.uniform(0.0, 1.0) < 0.5 else -1.0
            c = c + sign * off * n
            world[b, i] = (c[0], c[1], rng.uniform(0.1, 0.4))
        psi0 = np.pi / 2 + rng.uniform(-0.3, 0.3)
        nedx = 4.0 + rng.uniform(-1.0, 1.0)
        x0[b, 0], x0[b, 3], x0[b, 10], x0[b, 11] = psi0, 0.001, nedx, -5.0
        if moving:
            rv = np.random.default_rng([seed + b, 1])
            for i in range(4):
                d = w[i % 2 + 1] - w[i % 2]
                e = d / np.hypot(d[0], d[1])
                n = np.array([-e[1], e[0]])
                vel[b, i] = rv.uniform(-PF_DRIFT_ALONG, PF_DRIFT_ALONG) * e + rv.uniform(-PF_DRIFT_ACROSS, PF_DRIFT_ACROSS) * n
    out = dict(waypoints=np.tile(w[None], (B, 1, 1)), world=world, x0=x0)
    if moving:
        out["world_vel"] = vel
    return out


def predict_world(world, vel, chosen, N, dt, margin=PF_MISSION_OCP["margin"]):
    """The per-stage obstacle set a moving-world prepare writes (csrc/pf_guidance.hpp), in numpy: world [B,L,3], vel [B,L,2], chosen [B,K]
    (list index behind each slot, -1: parked) -> p [B,N+1,2K], lh [B,N,K].  p[k] = pos + ((double)k * dt) * vel, every product and sum rounded
    on its own; a parked slot is (1000, 1000) with velocity 0 and lh 0."""
    world, vel, chosen = np.asarray(world, dtype=float), np.asarray(vel, dtype=float), np.asarray(chosen, dtype=int)
    B, K = chosen.shape
    pos, v, lh0 = np.full((B, K, 2), 1000.0), np.zeros((B, K, 2)), np.zeros((B, K))
    bb, ss = np.nonzero(chosen >= 0)
    ii = chosen[bb, ss]
    pos[bb, ss], v[bb, ss] = world[bb, ii, :2], vel[bb, ii]
    lh0[bb, ss] = (world[bb, ii, 2] + 0.5) + margin
    kdt = (np.arange(N + 1, dtype=float) * dt)[None, :, None, None]
    p = (pos[:, None] + kdt * v[:, None]).reshape(B, N + 1, 2 * K)
    return p, np.tile(lh0[:, None], (1, N, 1))


# ---- missions of the obstacle-avoidance guidance model (usv_model_guidance_ca1; examples/scenario_sweep.py)
CA_MISSION_WAYPOINTS = np.array([[4.0, -5.0], [4.0, 25.0], [10.0, 30.0]])
CA_DRIFT = 0.3   # m/s: the survey's range for moving obstacles


def make_ca_worlds(B, L, rng):
    """L obstacles per scenario along the first leg (4,-5) -> (4,25): one every 25/L metres (jittered), up to
    1.5 m off the path to either side, radius 0.3..0.8 m - the reference scenario's density
    (usv_guidance_ca1/main.py: four obstacles on a 30 m leg), randomised."""
    y = -1.0 + (np.arange(L)[None, :] + rng.uniform(0.2, 0.8, (B, L))) * (25.0 / L)
    x = 4.0 + rng.uniform(-1.5, 1.5, (B, L))
    r = rng.uniform(0.3, 0.8, (B, L))
    return np.stack([x, y, r], axis=2)


def make_ca_missions(B, L, seed=0, moving=False):
    """B LiDAR scenarios drawn from numpy.random.default_rng(seed): dict(waypoints [3,2], pose [B,3] = (nedx, nedy, psi) - the vessel starts
    at (4 +- 1, -5), heading pi/2 +- 0.3 -, vel [B,2] = (0.7, 0), world [B,L,3] = (X, Y, R) of make_ca_worlds).
    moving=True adds world_vel [B,L,2]: every obstacle crosses the first leg (which runs along Y) at vX ~ U(-CA_DRIFT, CA_DRIFT), vY = 0,
    drawn from a stream of its own, default_rng([seed, 1]): every other field is the same bits with either value of `moving`."""
    rng = np.random.default_rng(seed)
    world = make_ca_worlds(B, L, rng)
    pose = np.column_stack([4.0 + rng.uniform(-1, 1, B), np.full(B, -5.0), np.full(B, np.pi / 2) + rng.uniform(-0.3, 0.3, B)])
    vel = np.column_stack([np.full(B, 0.7), np.zeros(B)])
    out = dict(waypoints=CA_MISSION_WAYPOINTS.copy(), pose=pose, vel=vel, world=world)
    if moving:
        rv = np.random.default_rng([seed, 1])
        out["world_vel"] = np.stack([rv.uniform(-CA_DRIFT, CA_DRIFT, (B, L)), np.zeros((B, L))], axis=2)
    return out


# ---- vessel encounters for usv_model_pf_ca behind guidance.PathFollowingFrontEnd.set_fleet: scenes of S vessels that are each other's
# moving obstacles (csrc/fleet_world.hpp)
def fleet_vessels(B, S):
    """[B, S-1]: the vessel behind fleet slot e of instance i = s S + a is s S + (e if e < a else e + 1)."""
    i, e = np.arange(B)[:, None], np.arange(S - 1)[None, :]
    a = i % S
    return i - a + np.where(e < a, e, e + 1)


def fleet_world(x0, S, radius=0.5):
    """The numpy restatement of the device's gather: x0 [B,14] -> (entries [B,S-1,3] = (X, Y, R), vel [B,S-1,2] = (vX, vY),
    separation [B,S-1]) of every instance's scene-mates; X, Y = x0_j[10], x0_j[11], sog = sqrt(u u + v v), vX = sog x0_j[2], vY = sog x0_j[1]
    (the model's own cos / sin of the course angle), separation = sqrt(dx dx + dy dy).  Every product and sum is rounded on its own, no
    trigonometric call: the same bits as the device."""
    x0 = np.asarray(x0, dtype=float)
    B = x0.shape[0]
    if S < 2 or B % S:
        raise ValueError("fleet_world: %d instances are not a whole number of scenes of %d (S >= 2)" % (B, S))
    xj = x0[fleet_vessels(B, S)]                                   # [B, S-1, 14]
    u, v = xj[..., 3], xj[..., 4]
    sog = np.sqrt(u * u + v * v)
    entries = np.stack([xj[..., 10], xj[..., 11], np.full(sog.shape, float(radius))], axis=2)
    vel = np.stack([sog * xj[..., 2], sog * xj[..., 1]], axis=2)
    dx, dy = xj[..., 10] - x0[:, None, 10], xj[..., 11] - x0[:, None, 11]
    return entries, vel, np.sqrt(dx * dx + dy * dy)


# Encounter geometry, settled with tools/pf_encounter_oracle.py (profiles/pf_encounter_oracle.txt) under hard obstacle rows, whose keep-out
# distance between two hulls of radius 0.5 is (0.5 + 0.5) + 0.2 = 1.2 m:
PF_ENC_LANE = 2.0            # m between neighbouring lanes, +- PF_ENC_LANE_JITTER per vessel
PF_ENC_LANE_JITTER = 0.2
PF_ENC_STAGGER = 0.5         # m: a vessel starts up to this far ahead of or behind its line
PF_ENC_CROSS_OFFSET = 3.0    # m: a crossing vessel starts this much farther from the crossing point than the one it crosses (4.3 s at 0.7 m/s)
PF_ENC_HEAD_ON_LATERAL = 1.1 # m: lateral offset of two opposing lanes (port to port), +- PF_ENC_LANE_JITTER per vessel: less than the 1.2 m, both swerve
PF_ENC_SPEED = 0.7
PF_ENC_KINDS = ("parallel", "crossing", "head_on")


def make_pf_encounters(scenes, S, seed=0, kind="parallel"):
    """scenes * S missions, scene s (instances s S .. s S + S - 1) drawn from numpy.random.default_rng(seed + s): a scene does not depend on
    the batch it is in.  Returns dict(waypoints [B,3,2], x0 [B,14], world [B,0,3] - no fixed obstacle: the scene's vessels are the obstacles).
    Every vessel sails a two-leg route at PF_ENC_SPEED from the start (u = 0.7; x0[1], x0[2] = sin / cos of the heading), vessel a of a
    scene, with lane l = a // 2 for the kinds that pair vessels up:
      "parallel"   all northwards side by side: (x, -5) -> (x, -1) -> (x + 1.5, 2) with x = 4 + a (PF_ENC_LANE +- jitter)
      "crossing"   even a northwards as above on x = 4 + l (lane); odd a westwards (9 + offset, y) -> (1, y) -> (-2, y + 1.5) with
                   y = -2 + l (lane): it reaches the crossing point PF_ENC_CROSS_OFFSET (+- stagger) metres of sailing after the northbound one
      "head_on"    even a northwards on x = 4 + 2 l (lane); odd a southwards (x', 3) -> (x', -1) -> (x' - 1.5, -4) on
                   x' = 4 + 2 l (lane) - PF_ENC_HEAD_ON_LATERAL: the two pass port to port and turn away from each other."""
    if kind not in PF_ENC_KINDS:
        raise ValueError("make_pf_encounters: kind must be one of %s" % (PF_ENC_KINDS,))
    B = scenes * S
    wp, x0 = np.zeros((B, 3, 2)), np.zeros((B, 14))
    for s in range(scenes):
        rng = np.random.default_rng(seed + s)
        for a in range(S):
            b = s * S + a
            jit = rng.uniform(-PF_ENC_LANE_JITTER, PF_ENC_LANE_JITTER)
            stag = rng.uniform(-PF_ENC_STAGGER, PF_ENC_STAGGER)
            lane = a // 2
            if kind == "parallel" or a % 2 == 0:
                x = 4.0 + (a * PF_ENC_LANE if kind == "parallel" else (2 * lane if kind == "head_on" else lane) * PF_ENC_LANE) + jit
                wp[b] = [[x, -5.0], [x, -1.0], [x + 1.5, 2.0]]
                start, psi = (x, -5.0 + stag), np.pi / 2
            elif kind == "crossing":
                y = -2.0 + lane * PF_ENC_LANE + jit
                wp[b] = [[9.0 + PF_ENC_CROSS_OFFSET, y], [1.0, y], [-2.0, y + 1.5]]
                start, psi = (7.0 + PF_ENC_CROSS_OFFSET + stag, y), np.pi
            else:
                x = 4.0 + 2 * lane * PF_ENC_LANE - PF_ENC_HEAD_ON_LATERAL + jit
                wp[b] = [[x, 3.0], [x, -1.0], [x - 1.5, -4.0]]
                start, psi = (x, 3.0 + stag), -np.pi / 2
            x0[b, 0], x0[b, 1], x0[b, 2], x0[b, 3] = psi, np.sin(psi), np.cos(psi), PF_ENC_SPEED
            x0[b, 10], x0[b, 11] = start
    return dict(waypoints=wp, x0=x0, world=np.zeros((B, 0, 3)))


# ---- vessel encounters for usv_model_guidance_ca1 behind guidance.GuidanceFrontEnd.set_fleet (csrc/ca_fleet_world.hpp); scenes and slots
# as fleet_vessels above
def ca_fleet_world(x0, S, radius=0.5):
    """The numpy restatement of the device's gather for the guidance model: x0 [B,8] = (u, v, ye, chie, psied, xned, yned, psi) ->
    (entries [B,S-1,3] = (X, Y, R), vel [B,S-1,2] = (vX, vY), separation [B,S-1]) of every instance's scene-mates; X, Y = x0_j[5], x0_j[6],
    vX = u cos psi - v sin psi, vY = u sin psi + v cos psi, separation = sqrt(dx dx + dy dy).  Every product and sum is rounded on its own:
    entries and separations are the device's bits, the velocities agree to 8 * 2^-52 * (|u| + |v|) (two libraries' sin / cos)."""
    x0 = np.asarray(x0, dtype=float)
    B = x0.shape[0]
    if S < 2 or B % S:
        raise ValueError("ca_fleet_world: %d instances are not a whole number of scenes of %d (S >= 2)" % (B, S))
    xj = x0[fleet_vessels(B, S)]                                   # [B, S-1, 8]
    u, v = xj[..., 0], xj[..., 1]
    s, c = np.sin(xj[..., 7]), np.cos(xj[..., 7])
    entries = np.stack([xj[..., 5], xj[..., 6], np.full(u.shape, float(radius))], axis=2)
    vel = np.stack([u * c + -(v * s), u * s + v * c], axis=2)
    dx, dy = xj[..., 5] - x0[:, None, 5], xj[..., 6] - x0[:, None, 6]
    return entries, vel, np.sqrt(dx * dx + dy * dy)


# ---- exchanged plans for both front ends' fleets (csrc/fleet_plan.hpp): a scene-mate's slot follows the mate's own planned path
FLEET_PLAN_POS = {"usv_model_pf_ca": (10, 11), "usv_model_guidance_ca1": (5, 6)}   # the position pair of a state


def fleet_plan_stages(p, x, chosen, S, n_fixed, status, finish_tick, pos=(10, 11), q=None):
    """The numpy restatement of the device's plan kernel (usv_pf_fleet_plans / usv_guidance_fleet_plans).  p [B,N+1,2K]: the stages as the
    constant-velocity prepare left them; x [B,N+1,nx]: the iterate, one hand-over old; chosen [B,K]: the list index behind each slot
    (-1: parked; every slot of an instance that does not stream this tick); status [B] of the last solve; finish_tick [B] as this prepare
    left it (>= 0: the mission is over); pos: the model's position states (FLEET_PLAN_POS); q [B,K,2]: the slots' stage-0 positions
    (default: stage 0 of p).  -> (p [B,N+1,2K], source [B,K]: the vessel behind each plan-fed slot, -1: none).
    Slot s of instance i with c = chosen[i,s] >= n_fixed has the source j = fleet_vessels(B, S)[i, c - n_fixed], used when finish_tick[j] < 0
    and status[j] == 0.  With P_k = x[j,k,pos] and e = q - P_1: stage k = 1 .. N-1 becomes P_{k+1} + e, stage N becomes
    (P_N + (P_N - P_{N-1})) + e; stage 0 and every other slot keep their bits.  Sums and differences only, each rounded on its own: the
    device's bits."""
    p, x, chosen = np.array(p, dtype=float), np.asarray(x, dtype=float), np.asarray(chosen, dtype=int)
    status, finish_tick = np.asarray(status, dtype=int), np.asarray(finish_tick, dtype=int)
    B, K = chosen.shape
    N = p.shape[1] - 1
    if N < 2:
        raise ValueError("fleet_plan_stages: a plan needs N >= 2")
    if S < 2 or B % S:
        raise ValueError("fleet_plan_stages: %d instances are not a whole number of scenes of %d (S >= 2)" % (B, S))
    mates = fleet_vessels(B, S)
    e_idx = chosen - n_fixed
    has = (chosen >= n_fixed) & (e_idx < S - 1)
    j = np.where(has, mates[np.arange(B)[:, None], np.clip(e_idx, 0, S - 2)], -1)
    ok = has & (finish_tick[np.clip(j, 0, B - 1)] < 0) & (status[np.clip(j, 0, B - 1)] == 0)
    source = np.where(ok, j, -1)
    bb, ss = np.nonzero(ok)
    if bb.size == 0:
        return p, source
    P = x[source[bb, ss]][:, :, list(pos)]                              # [n, N+1, 2]
    slots = p.reshape(B, N + 1, K, 2)
    q0 = slots[bb, 0, ss] if q is None else np.asarray(q, dtype=float).reshape(B, K, 2)[bb, ss]
    e = q0 - P[:, 1]
    slots[bb[:, None], np.arange(1, N)[None, :], ss[:, None]] = P[:, 2:N + 1] + e[:, None]
    slots[bb, N, ss] = (P[:, N] + (P[:, N] - P[:, N - 1])) + e
    return slots.reshape(B, N + 1, 2 * K), source


# Encounter geometry, settled with tools/guidance_encounter_oracle.py (profiles/guidance_encounter_oracle.txt) under this model's SOFT
# obstacle rows, whose keep-out distance between two hulls of radius 0.5 is 0.5 + 0.5 = 1.0 m:
CA_ENC_LANE = 2.0            # m between neighbouring lanes, +- CA_ENC_LANE_JITTER per vessel
CA_ENC_LANE_JITTER = 0.2
CA_ENC_STAGGER = 0.5         # m: a vessel starts up to this far ahead of or behind its line
CA_ENC_CROSS_OFFSET = 3.0    # m: a crossing vessel starts this much farther from the crossing point than the one it crosses (4.3 s at 0.7 m/s)
CA_ENC_HEAD_ON_LATERAL = 1.1 # m: lateral offset of two opposing lanes (port to port), +- CA_ENC_LANE_JITTER per vessel
CA_ENC_SPEED = 0.7           # (the node's speed set-point, D_SPEED)
CA_ENC_KINDS = ("parallel", "crossing", "head_on")
CA_ENC_OCP = dict(N=100, K=8, dt=0.05, max_radius=100.0)   # examples/scenario_sweep.py --resident: the reference's deployment


def make_ca_encounters(scenes, S, seed=0, kind="parallel"):
    """scenes * S missions, scene s (instances s S .. s S + S - 1) drawn from numpy.random.default_rng(seed + s): a scene does not depend on
    the batch it is in.  Returns dict(waypoints [B,3,2], pose [B,3] = (nedx, nedy, psi), vel [B,2] = (CA_ENC_SPEED, 0), x0 [B,8] (the two in
    the model's state order), world [B,0,3] - no fixed obstacle: the scene's vessels are the obstacles).  Every vessel sails a two-leg route,
    vessel a of a scene, with lane l = a // 2 for the kinds that pair vessels up:
      "parallel"   all northwards side by side: (x, -5) -> (x, -1) -> (x + 1.5, 2) with x = 4 + a (CA_ENC_LANE +- jitter)
      "crossing"   even a northwards as above on x = 4 + l (lane); odd a westwards (9 + offset, y) -> (1, y) -> (-2, y + 1.5) with
                   y = -2 + l (lane): it reaches the crossing point CA_ENC_CROSS_OFFSET (+- stagger) metres of sailing after the northbound one
      "head_on"    even a northwards on x = 4 + 2 l (lane); odd a southwards (x', 3) -> (x', -1) -> (x' - 1.5, -4) on
                   x' = 4 + 2 l (lane) - CA_ENC_HEAD_ON_LATERAL: the two pass port to port and turn away from each other."""
    if kind not in CA_ENC_KINDS:
        raise ValueError("make_ca_encounters: kind must be one of %s" % (CA_ENC_KINDS,))
    B = scenes * S
    wp, pose = np.zeros((B, 3, 2)), np.zeros((B, 3))
    for s in range(scenes):
        rng = np.random.default_rng(seed + s)
        for a in range(S):
            b = s * S + a
            jit = rng.uniform(-CA_ENC_LANE_JITTER, CA_ENC_LANE_JITTER)
            stag = rng.uniform(-CA_ENC_STAGGER, CA_ENC_STAGGER)
            lane = a // 2
            if kind == "parallel" or a % 2 == 0:
                x = 4.0 + (a * CA_ENC_LANE if kind == "parallel" else (2 * lane if kind == "head_on" else lane) * CA_ENC_LANE) + jit
                wp[b] = [[x, -5.0], [x, -1.0], [x + 1.5, 2.0]]
                pose[b] = (x, -5.0 + stag, np.pi / 2)
            elif kind == "crossing":
                y = -2.0 + lane * CA_ENC_LANE + jit
                wp[b] = [[9.0 + CA_ENC_CROSS_OFFSET, y], [1.0, y], [-2.0, y + 1.5]]
                pose[b] = (7.0 + CA_ENC_CROSS_OFFSET + stag, y, np.pi)
            else:
                x = 4.0 + 2 * lane * CA_ENC_LANE - CA_ENC_HEAD_ON_LATERAL + jit
                wp[b] = [[x, 3.0], [x, -1.0], [x - 1.5, -4.0]]
                pose[b] = (x, 3.0 + stag, -np.pi / 2)
    vel = np.column_stack([np.full(B, CA_ENC_SPEED), np.zeros(B)])
    x0 = np.zeros((B, 8))
    x0[:, 0:2], x0[:, 5:8] = vel, pose
    return dict(waypoints=wp, pose=pose, vel=vel, x0=x0, world=np.zeros((B, 0, 3)))


# ---- the two-layer control stack (guidance.Cascade; csrc/cascade.hpp): guidance layer -> low-level NMPC (usv_model_low_level) -> vessel.
# The numpy restatement of the coupling arithmetic, what the device's kernels usv_cascade_refs / usv_cascade_step are held against.
CASCADE_C = 0.78          # the starboard thruster's factor of usv_model_low_level
CASCADE_LL_OCP = dict(N=100, dt=0.01, ratio=5, num_steps=1)   # the reference's deployment: low level at 100 Hz, guidance at 20 Hz


def _dof3(c, u, v, r, Tp, Ts):
    """(udot, vdot, rdot) of the 3-DOF block (usv_models._dof3_sym in numpy), vectorised"""
    m, Iz, Bw = 30.0, 4.1, 0.41
    Xud, Yvd, Yrd, Nvd, Nrd = -2.25, -23.13, -1.31, -16.41, -2.79
    Yvv, Yvr, Nrv, Nrr = -99.99, -5.49, -8.8, -3.49
    fast = u > 1.25
    Xu, Xuu = np.where(fast, 64.55, -25.0), np.where(fast, -70.92, 0.0)
    au, av, ar = np.abs(u), np.abs(v), np.abs(r)
    Nr = -0.52 * np.sqrt(u * u + v * v)
    a = Yrd + Nvd
    fu = ((Tp + c * Ts) - (-m + 2.0 * Yvd) * v - a * r * r - (-Xu * u - Xuu * au * u)) / (m - Xud)
    fv = (-(m - Xud) * u * r - (-_CY * av - Yvv * av - Yvr * ar) * v) / (m - Yvd)
    fr = ((Tp - c * Ts) * (Bw / 2.0) - (-2.0 * Yvd * u * v - a * r * u + Xud * u * r) - (-Nr * r - Nrv * av * r - Nrr * ar * r)) / (Iz - Nrd)
    return fu, fv, fr


def _cascade_rhs(s, thr, c):
    psi, u, v, r = s[:, 2], s[:, 3], s[:, 4], s[:, 5]
    sp, cp = np.sin(psi), np.cos(psi)
    fu, fv, fr = _dof3(c, u, v, r, thr[:, 0], thr[:, 1])
    return np.stack([u * cp - v * sp, u * sp + v * cp, r, fu, fv, fr], axis=1)


def cascade_plant_step(s, thr, T, num_steps=1, c=CASCADE_C):
    """One period T of the vessel s [B,6] = (nedx, nedy, psi, u, v, r) under the held thrusts thr [B,2] = (Tport, Tstbd): num_steps RK4
    steps, summed in the device's order (k1 + 2 k2 + 2 k3, then + k4).  The device fuses its multiply-adds: agreement to 1e-12."""
    s, thr = np.array(s, dtype=float).reshape(-1, 6), np.asarray(thr, dtype=float).reshape(-1, 2)
    h = T / float(num_steps)
    for _ in range(int(num_steps)):
        k = _cascade_rhs(s, thr, c)
        acc = k
        k = _cascade_rhs(s + 0.5 * h * k, thr, c)
        acc = acc + 2.0 * k
        k = _cascade_rhs(s + 0.5 * h * k, thr, c)
        acc = acc + 2.0 * k
        k = _cascade_rhs(s + h * k, thr, c)
        s = s + (h / 6.0) * (acc + k)
    return s


def cascade_ll_inputs(s, past, psi_des, u_des):
    """The low-level node's input side (nmpc_low_level.cpp:177-245): vessel s [B,6], past thrusts [B,2], set-points [B] ->
    (x0 [B,8] = (psi, sin psi, cos psi, u (0 -> 0.001), v, r, past thrusts), yref row [B,10] = (psi_des, sin, cos, u_des, 0 ..)); yref_e is
    the row's first eight entries."""
    s, past = np.asarray(s, dtype=float).reshape(-1, 6), np.asarray(past, dtype=float).reshape(-1, 2)
    psi_des, u_des = np.asarray(psi_des, dtype=float).reshape(-1), np.asarray(u_des, dtype=float).reshape(-1)
    psi = s[:, 2]
    u = np.where(s[:, 3] == 0.0, 0.001, s[:, 3])
    x0 = np.column_stack([psi, np.sin(psi), np.cos(psi), u, s[:, 4], s[:, 5], past[:, 0], past[:, 1]])
    yref = np.zeros((len(psi_des), 10))
    yref[:, 0], yref[:, 1], yref[:, 2], yref[:, 3] = psi_des, np.sin(psi_des), np.cos(psi_des), u_des
    return x0, yref


def cascade_ll_outputs(x1, psi_des, u_des, s):
    """The low-level node's output side (:256-285) from stage 1 of its iterate x1 [B,8]: (published thrusts [B,2] - zero where u_des == 0 -,
    past thrusts [B,2] = x1[6:8] regardless, e_u, e_psi [B] float32 against the state s the solve saw)."""
    x1, s = np.asarray(x1, dtype=float).reshape(-1, 8), np.asarray(s, dtype=float).reshape(-1, 6)
    psi_des, u_des = np.asarray(psi_des, dtype=float).reshape(-1), np.asarray(u_des, dtype=float).reshape(-1)
    past = x1[:, 6:8].copy()
    thr = np.where((u_des == 0.0)[:, None], 0.0, past)
    u = np.where(s[:, 3] == 0.0, 0.001, s[:, 3])
    return thr, past, (u_des - u).astype(np.float32), (psi_des - s[:, 2]).astype(np.float32)


def cascade_guidance_tick(tick, ratio):
    """Low-level tick `tick` (from 0) begins with a guidance solve"""
    return tick % ratio == 0


def cascade_hands_over(tick, ratio):
    """... and the plant step of tick `tick` writes the vessel's state into the guidance layer's x0 when the NEXT tick is a guidance tick"""
    return (tick + 1) % ratio == 0
