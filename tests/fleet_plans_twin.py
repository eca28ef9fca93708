"""What the two GPU test files of exchanged plans share (tests/test_gpu_pf_fleet_plans.py, tests/test_gpu_guidance_fleet_plans.py): the TWIN.
Handle A has plans on.  Handle B has the fleet on and plans off, and a host that does by hand what the plan kernel does on the device: it
reads x, status and the front-end state back before each prepare, keeps the rule for when a plan is usable (include/usvmpc.h) in a few lines
of its own, builds p with scenario.fleet_plan_stages after the prepare and writes it with set_all("p").  The two must agree bit for bit."""
import numpy as np

from mpc_collisionavoidance_amd import scenario

NONE, SOLVED, SHIFTED = 0, 1, 2


class HostRule:
    """The table of include/usvmpc.h, kept by the twin's host: a plan is usable by the one prepare that finds the iterate solved and handed
    over exactly once."""

    def __init__(self):
        self.state = NONE

    def solved(self):
        self.state = SOLVED

    def handed_over(self):
        self.state = SHIFTED if self.state == SOLVED else NONE

    def lost(self):
        self.state = NONE

    def use(self):
        ok = self.state == SHIFTED
        if ok:
            self.state = NONE
        return ok


def chosen_from_stage0(p0, world, tol):
    """[B, K]: the list index behind each slot, -1 for a parked one, read off stage 0 of p ([B, 2K]) against the world list ([B, L, 3]) the
    prepare selected from.  tol 0: the path-following front end copies the entry's position; the guidance front end rounds it through
    float32 (tol 1e-4; the entries of these scenes lie decimetres apart)."""
    B = p0.shape[0]
    slots = p0.reshape(B, -1, 2)
    d = np.abs(slots[:, :, None, :] - world[:, None, :, :2]).max(axis=3)          # [B, K, L]
    hit = d <= tol
    assert (hit.sum(axis=2) <= 1).all(), "two world entries on one spot"
    return np.where(hit.any(axis=2), hit.argmax(axis=2), -1)


class Twin:
    """cfg: dict(S, n_fixed, pos, tol, finish (fe -> finish_tick [B]), streams_before (the instance streams when its mission was not over
    BEFORE the prepare - the guidance tick; else AFTER it - the path-following prepare))"""

    def __init__(self, a, b, cfg):
        (self.sa, self.fa), (self.sb, self.fb), self.cfg = a, b, cfg
        self.rule = HostRule()
        self.fed = 0
        self.launches = 0

    def prepare(self, what, plans_on=True):
        """both prepare; B's host applies the plans.  -> (the constant-velocity p, source [B, K] or None when no plan was usable)"""
        c = self.cfg
        x, status, fin_before = self.sb.get_all("x"), self.sb.get_int("status"), c["finish"](self.fb)
        self.fa.prepare(), self.fb.prepare()
        p_cv = self.sb.get_all("p")
        K = p_cv.shape[2] // 2
        src = None
        if plans_on and self.rule.use():
            fin_after = c["finish"](self.fb)
            streams = (fin_before if c["streams_before"] else fin_after) < 0
            chosen = chosen_from_stage0(p_cv[:, 0], self.fb.world()[0], c["tol"])
            chosen[~streams] = -1
            p_new, src = scenario.fleet_plan_stages(p_cv, x, chosen, c["S"], c["n_fixed"], status, fin_after, pos=c["pos"])
            self.sb.set_all("p", p_new)
            self.fed += int((src >= 0).sum())
            self.launches += 1
        pa, pb = self.sa.get_all("p"), self.sb.get_all("p")
        assert pa.tobytes() == pb.tobytes(), (what, "p", int((pa != pb).any(axis=(1, 2)).sum()))
        assert self.sa.get_all("lh").tobytes() == self.sb.get_all("lh").tobytes(), (what, "lh")
        st = self.fa.fleet_plan_state()
        assert np.array_equal(st["source"], src if src is not None else np.full((p_cv.shape[0], K), -1)), (what, "source")
        assert st["plan_fed"] == self.fed and st["plan_launches"] == self.launches, (what, st["plan_fed"], self.fed, st["plan_launches"], self.launches)
        return p_cv, src

    def solved(self):
        self.rule.solved()

    def handed_over(self):
        self.rule.handed_over()
