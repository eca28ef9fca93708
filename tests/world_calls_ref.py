"""The front ends' resident world list, stated once for the plan on the CPU (tests/test_world_plan.py drives csrc/world_plan.hpp through
tests/world_plan_harness.cpp) and for the library on the device (tests/test_gpu_world_calls.py drives the C ABI): the refusals' words, one
scripted pass through the transitions with what every call is expected to do and leave behind, and the list's layout in numpy.  Everything
here is written out by hand from include/usvmpc.h and the entry points as they stood before world_plan.hpp; nothing is taken from the code
under test."""
import numpy as np

KINDS = ("guidance", "pf")
B, S = 6, 3

# WorldDo (csrc/world_plan.hpp)
NOTHING, UPLOAD_LIST, RELAYOUT, UPLOAD_VEL, MERGE_VEL, STEP, READ, FLEET_STATE = range(8)

# ---- the refusals, word for word.  {who}: the call, "guidance_world", "pf_fleet", ..
_TRACKS = "{who}: option \"obstacle_tracks\" is on and the tracks own p; switch it off first"
REFUSALS = {
    "guidance": {
        "wrong_model": "{who}: the guidance front end belongs to usv_model_guidance_ca1",
        "before_reset": "{who}: usvmpc_guidance_reset must be called first",
        "fleet_no_list": "guidance_fleet: no world list yet (usvmpc_guidance_world first; an empty one will do)",
        "no_list": "{who}: no world list yet (usvmpc_guidance_world first)",
        "vel_null_fleet": "guidance_world_vel: a fleet is on and its world moves; switch it off first (usvmpc_guidance_fleet with scene_size 0)",
        "at_rest": "guidance_world_step: the world is at rest (usvmpc_guidance_world_vel first)",
    },
    "pf": {
        "wrong_model": "the path-following front end (usvmpc_pf_*) belongs to usv_model_pf_ca",
        "before_reset": "usvmpc_pf_reset must be called first",
        "fleet_no_list": "pf_fleet: usvmpc_pf_reset and a world list (usvmpc_pf_world; an empty one will do) come first",
        "no_list": "{who}: no world list yet (usvmpc_pf_world first)",
        "vel_null_fleet": "pf_world_vel: a fleet is on and its world moves; switch it off first (usvmpc_pf_fleet with scene_size 0)",
        "at_rest": "pf_world_step: the world is at rest (usvmpc_pf_world_vel first)",
    },
}
for _k in KINDS:
    REFUSALS[_k].update({
        "n_world": "{who}: n_world must lie in 0..64",
        "null_list": "{who}: null world list",
        "radius_nan": "{who}: max_radius is NaN",
        "entry_nan": "{who}: entry {i} is NaN",
        "fleet_owns": "{who}: a fleet is on and owns {slots} entries of the list: n_world must lie in 0..{most}",
        "tracks": _TRACKS,
        "not_finite": "{who}: entry {i} is not finite",
        "T": "{who}: T is not finite",
        "scene_negative": "{who}: scene_size must not be negative",
        "scenes": "{who}: the batch of {B} is not a whole number of scenes of {S}",
        "fits": "{who}: {n_fixed} fixed entries and {slots} fleet entries exceed the 64 of a world list",
        "radius": "{who}: radius must be finite and not negative",
    })

PREFIX = {"guidance": "guidance_", "pf": "pf_"}
CALLS = {"world": "world", "vel": "world_vel", "step": "world_step", "read": "world_read", "fleet": "fleet", "fstate": "fleet_state"}


def refusal(kind, call, key, **kw):
    """the message of `call` ("world", "vel", "step", "read", "fleet", "fstate") on a front end of `kind`"""
    return REFUSALS[kind][key].format(who=PREFIX[kind] + CALLS[call], **kw)


def relayout_ref(w0, v0, n0f, f0, fixed, n1f, f1):
    """csrc/fleet_world.hpp, fleet_relayout, for one instance: the fixed entries (new ones when given; their velocities kept only when the
    world moved and their count is unchanged), the fleet slots behind them (those there are stay, new ones are parked at rest)"""
    w1, v1 = np.zeros((n1f + f1, 3)), np.zeros((n1f + f1, 2))
    w1[:n1f] = fixed if fixed is not None else w0[:n1f]
    if v0 is not None and n1f == n0f:
        v1[:n1f] = v0[:n1f]
    for e in range(f1):
        if e < f0:
            w1[n1f + e] = w0[n0f + e]
            v1[n1f + e] = v0[n0f + e] if v0 is not None else 0.0
        else:
            w1[n1f + e] = (1000.0, 1000.0, 0.0)
    return w1, v1


def _gp(g, p):
    return {"guidance": g, "pf": p}


def _act(what=NOTHING, need=0, grow=0, need_vel=0, grow_vel=0, n0=0, f0=0, n1_fixed=0, f1=0, new_fixed=0, n=0, nvel=0, vel_on_device=0,
         host_answer=0, make_front_end=0, make_tracks=0, make_sep=0, apply_static=0):
    return dict(locals())


def _st(nworld, nfixed, moving, fleet_S, want_static, list_cap, vel_cap, **more):
    return dict(set=1, nworld=nworld, nfixed=nfixed, moving=moving, fleet_S=fleet_S, want_static=want_static, list_cap=list_cap, vel_cap=vel_cap,
                **more)


# ---- one pass through the transitions: B = 6, lists of 2, 3 and 0 entries, scenes of 2 and 3.  Every step: the call and its arguments
# (world: n entries, max_radius; vel: given?, predict; fleet: scene size, radius; step: T), then either `err` (a key of REFUSALS and its
# numbers: the call is refused and nothing changes) or `act` (what the carrier is told) and `state` (what stands afterwards).  A value that
# differs between the front ends is a dict by kind.  want_static is for option "pf_predict" 1.  Sizes are doubles: a list of n entries needs
# 6 n 3, its velocities 6 n 2; a buffer is replaced (grow) only when the need exceeds its capacity - or, the velocities', when there is none.
SCRIPT = [
    # a fresh list: at rest.  The guidance front end makes its slot tracks now, the path-following one its own buffers (the call may come
    # ahead of its reset)
    dict(call="world", n=2, radius=50.0,
         act=_act(UPLOAD_LIST, need=36, grow=1, make_front_end=_gp(0, 1), make_tracks=_gp(1, 0)),
         state=_st(2, 0, 0, 0, 1, 36, 0, max_radius=50.0, has_vel=0, tracks=_gp(1, 0), sep=0)),
    # no fleet yet: guidance answers 1e300 / -1 from the host, path-following reads the buffers its reset filled
    dict(call="fstate", act=_act(FLEET_STATE, host_answer=_gp(1, 0)), state=_st(2, 0, 0, 0, 1, 36, 0)),
    dict(call="step", T=0.5, err=("at_rest", {})),
    # velocities: the world moves and is predicted ("static_obstacles" off); path-following makes its slot tracks now
    dict(call="vel", given=1, predict=1,
         act=_act(UPLOAD_VEL, need=24, grow=1, n=2, nvel=2, make_tracks=_gp(0, 1), apply_static=1),
         state=_st(2, 0, 1, 0, 0, 36, 24, has_vel=1, tracks=1, predict=_gp(1, 0))),
    # a list of the same count over a moving world keeps velocities and keeps moving
    dict(call="world", n=2, radius=60.0, act=_act(UPLOAD_LIST, need=36, make_front_end=_gp(0, 1)), state=_st(2, 0, 1, 0, 0, 36, 24, max_radius=60.0)),
    # another count goes to rest and asks for static
    dict(call="world", n=3, radius=60.0, act=_act(UPLOAD_LIST, need=54, grow=1, make_front_end=_gp(0, 1), apply_static=1),
         state=_st(3, 0, 0, 0, 1, 54, 24)),
    dict(call="vel", given=1, predict=1, act=_act(UPLOAD_VEL, need=36, grow=1, n=3, nvel=3, apply_static=1), state=_st(3, 0, 1, 0, 0, 54, 36)),
    # ... then NULL: back to rest, nothing for the carrier to do
    dict(call="vel", given=0, predict=0, act=_act(NOTHING, apply_static=1), state=_st(3, 0, 0, 0, 1, 54, 36, predict=_gp(1, 0))),
    # a fleet over a world at rest: 3 fixed entries and 2 slots; the world moves from now on.  Guidance: predict becomes 1
    dict(call="fleet", S=3, radius=0.4,
         act=_act(RELAYOUT, need=90, grow=1, need_vel=60, grow_vel=1, n0=3, f0=0, n1_fixed=3, f1=2, make_sep=_gp(1, 0), apply_static=1),
         state=_st(5, 3, 1, 3, 0, 90, 60, fleet_radius=0.4, predict=_gp(1, 0), sep=_gp(1, 0))),
    dict(call="fstate", act=_act(FLEET_STATE), state=_st(5, 3, 1, 3, 0, 90, 60)),
    # off: cut back to the fixed entries, nfixed stays, the world stays moving, "static_obstacles" is not asked for
    dict(call="fleet", S=0, radius=0.4, act=_act(RELAYOUT, need=54, need_vel=36, n0=5, f0=2, n1_fixed=3, f1=0),
         state=_st(3, 3, 1, 0, 0, 90, 60)),
    # off when off: nothing at all (a scene of 1 is no fleet either)
    dict(call="fleet", S=0, radius=0.4, act=_act(NOTHING), state=_st(3, 3, 1, 0, 0, 90, 60)),
    dict(call="fleet", S=1, radius=0.4, act=_act(NOTHING), state=_st(3, 3, 1, 0, 0, 90, 60)),
    # velocities held still inside the horizon: guidance's choice is stored (static again), path-following has option "pf_predict" for it
    dict(call="vel", given=1, predict=0, act=_act(UPLOAD_VEL, need=36, n=3, nvel=3, apply_static=1),
         state=_st(3, 3, 1, 0, _gp(1, 0), 90, 60, predict=0)),
    # a fleet over a moving world keeps that choice
    dict(call="fleet", S=2, radius=0.3, act=_act(RELAYOUT, need=72, need_vel=48, n0=3, f0=0, n1_fixed=3, f1=1, apply_static=1),
         state=_st(4, 3, 1, 2, _gp(1, 0), 90, 60, fleet_radius=0.3, predict=0)),
    # a larger scene while a fleet is on: the slot there is stays
    dict(call="fleet", S=3, radius=0.4, act=_act(RELAYOUT, need=90, need_vel=60, n0=4, f0=1, n1_fixed=3, f1=2, apply_static=1),
         state=_st(5, 3, 1, 3, _gp(1, 0), 90, 60, fleet_radius=0.4)),
    # a list while a fleet is on: the fixed entries only
    dict(call="world", n=2, radius=70.0, act=_act(RELAYOUT, need=72, need_vel=48, n0=5, f0=2, n1_fixed=2, f1=2, new_fixed=1),
         state=_st(4, 2, 1, 3, _gp(1, 0), 90, 60, max_radius=70.0)),
    # velocities while a fleet is on: [B][nfixed][2] merged into the head of every row, not an upload
    dict(call="vel", given=1, predict=1, act=_act(MERGE_VEL, need=24, n=4, nvel=2, apply_static=1),
         state=_st(4, 2, 1, 3, 0, 90, 60, predict=_gp(1, 0))),
    dict(call="vel", given=0, predict=1, err=("vel_null_fleet", {})),
    dict(call="world", n=63, radius=70.0, err=("fleet_owns", dict(slots=2, most=62))),
    dict(call="step", T=0.25, act=_act(STEP, n=4), state=_st(4, 2, 1, 3, 0, 90, 60)),
    dict(call="fleet", S=0, radius=0.4, act=_act(RELAYOUT, need=36, need_vel=24, n0=4, f0=2, n1_fixed=2, f1=0), state=_st(2, 2, 1, 0, 0, 90, 60)),
    # empty lists: another count, so at rest - and an empty list moves too
    dict(call="world", n=0, radius=70.0, act=_act(UPLOAD_LIST, make_front_end=_gp(0, 1), apply_static=1), state=_st(0, 2, 0, 0, 1, 90, 60)),
    dict(call="vel", given=1, predict=1, act=_act(UPLOAD_VEL, apply_static=1), state=_st(0, 2, 1, 0, 0, 90, 60, has_vel=1)),
    dict(call="step", T=0.1, act=_act(NOTHING), state=_st(0, 2, 1, 0, 0, 90, 60)),
]


def pick(v, kind):
    return v[kind] if isinstance(v, dict) else v


def call_data(i, shape):
    """the caller's array of step i: distinct finite values"""
    return 100.0 * i + np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) / 8.0


class WorldModel:
    """What usvmpc_*_world_read returns after every step of SCRIPT: the list [B][nworld][3] and its velocities [B][nworld][2] (zeros while
    the world is at rest), carried along in numpy from the step's `act` as written above."""

    def __init__(self):
        self.world, self.vel, self.moving = np.zeros((B, 0, 3)), np.zeros((B, 0, 2)), False

    def apply(self, step, kind, data):
        a = step["act"]
        what = a["what"]
        moving = bool(step["state"]["moving"])
        if what == UPLOAD_LIST:
            self.world = data.copy()
            if not (self.moving and moving):        # (kept only over a moving world that stays one: the same count)
                self.vel = np.zeros(data.shape[:2] + (2,))
        elif what == UPLOAD_VEL:
            self.vel = data.copy()
        elif what == RELAYOUT:
            n0f = a["n0"] - a["f0"]
            out = [relayout_ref(self.world[b], self.vel[b] if self.moving else None, n0f, a["f0"], data[b] if a["new_fixed"] else None,
                                a["n1_fixed"], a["f1"]) for b in range(B)]
            self.world, self.vel = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
        elif what == MERGE_VEL:
            self.vel[:, :a["nvel"]] = data
        elif what == STEP:
            self.world[:, :, :2] = self.world[:, :, :2] + step["T"] * self.vel     # (obstacle_tracks.hpp, track_step: each rounded on its own)
        self.moving = moving

    def read(self):
        return self.world, self.vel if self.moving else np.zeros_like(self.vel)
