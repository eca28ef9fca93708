"""numpy restatement of the path-following front end over a MOVING world, on top of tests/pf_frontend_ref.PfRef (which selects, on the
current positions, exactly as for a world at rest), written from the issue's statement - not from csrc/pf_guidance.hpp, which the tests
compare against it:

    slot s holds list entry i:   p[k][2s + c] = world[i][c] + ((double)k * dt) * wvel[i][c]   k = 0 .. N,  c = 0, 1
                                 lh[k][s]     = (R_i + 0.5) + margin                          k = 0 .. N-1
    a parked slot:               (1000, 1000), velocity 0, lh 0
    world step:                  world[i][c] <- world[i][c] + T * wvel[i][c]                  R untouched

Every product and sum is rounded on its own (numpy does not fuse).  Instances whose mission is over keep their p and lh."""
import numpy as np

from tests import pf_frontend_ref as R


def stages(world, wvel, chosen, N, dt, margin):
    """One instance: world [L,3], wvel [L,2], chosen [K] -> p [N+1, 2K], lh [N, K]"""
    K = len(chosen)
    p, lh = np.zeros((N + 1, 2 * K)), np.zeros((N, K))
    for s, i in enumerate(chosen):
        for k in range(N + 1):
            for c in range(2):
                p[k, 2 * s + c] = 1000.0 + (float(k) * dt) * 0.0 if i < 0 else world[i, c] + (float(k) * dt) * wvel[i, c]
        lh[:, s] = 0.0 if i < 0 else (world[i, 2] + R.BOAT_RADIUS) + margin
    return p, lh


class PfMovingRef(R.PfRef):
    def __init__(self, B, N, K, dt, margin=0.2):
        super().__init__(B, N, K, margin)
        self.dt = dt
        self.p = np.zeros((B, N + 1, 2 * K))
        self.lh = np.zeros((B, N, K))
        self.wvel = np.zeros((B, 0, 2))

    def set_world(self, world, max_radius=100.0, vel=None):
        super().set_world(world, max_radius)
        self.world = self.world.copy()
        L = self.world.shape[1]
        if vel is None:
            self.wvel = np.zeros((self.B, L, 2))
        else:
            v = np.asarray(vel, dtype=float)
            self.wvel = (np.tile(v[None], (self.B, 1, 1)) if v.ndim == 2 else v.reshape(self.B, L, 2)).copy()

    def prepare(self, vel=None, pose=None):
        super().prepare(vel, pose)
        for b in range(self.B):
            if self.phase[b] != R.OVER:
                self.p[b], self.lh[b] = stages(self.world[b], self.wvel[b], self.chosen[b], self.N, self.dt, self.margin)

    def step_world(self, T):
        self.world[:, :, :2] = self.world[:, :, :2] + T * self.wvel


def make_world(B, L, rng, vmax=0.5):
    """L obstacles about the scripted poses of pf_frontend_ref.scripted_sequence (some beyond the 12 m the tests see), velocities up to
    +-vmax m/s"""
    w = np.concatenate([rng.uniform(-2.0, 10.0, (B, L, 1)), rng.uniform(-8.0, 8.0, (B, L, 1)), rng.uniform(0.1, 0.6, (B, L, 1))], axis=2)
    if L >= 3:
        w[:, 2, :2] += 30.0        # never visible at max_radius 12
    return w, rng.uniform(-vmax, vmax, (B, L, 2))
