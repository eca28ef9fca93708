// world_plan.hpp — a front end's resident world list (include/usvmpc.h: usvmpc_guidance_world / _world_vel / _world_step / _world_read /
// _fleet / _fleet_state and the usvmpc_pf_* calls of the same names): what each call refuses, what it does to the list and what the list is
// afterwards, as host-only code.  No HIP header and no device pointer: usvmpc.hip's entry points ask WorldPlan to judge a call, carry_world
// carries out the WorldAct it answers with, and commit() makes the new state stand once that has succeeded; tests/world_plan_harness.cpp
// drives the same code from a command line (tests/test_world_plan.py).  The list's layout with a fleet on (fixed entries, fleet slots behind
// them, what a relayout keeps) is fleet_world.hpp's and is not restated here.
//
// A handle has one model, so at most one front end and ONE world.  The two front ends follow the same rules; the few places where they differ
// are the rows of WorldKind, and nothing else differs.
#pragma once

#include <cstddef>
#include <string>

#include "ca_guidance.hpp"
#include "fleet_world.hpp"
#include "pf_guidance.hpp"

namespace usv {

constexpr int WORLD_LMAX = 64; // entries of a world list, fixed and fleet together
static_assert(GUIDANCE_LMAX == WORLD_LMAX && PF_LMAX == WORLD_LMAX && FLEET_LMAX == WORLD_LMAX, "one list limit for both front ends and the fleet's layout");

// One row per front end.  "inherited": the two copies of the entry points this header replaced differed so; nobody designed it, a caller may
// depend on it, and a later change may decide it.
struct WorldKind {
    const char *prefix;        // who speaks in a message: "guidance_" + "world", ..
    const char *world_call;    // the call that gives a list (+ "_vel": the one that gives velocities)
    const char *fleet_call;    // the call named in "switch it off first (.. with scene_size 0)"
    const char *reset_call;    // the front end's reset
    const char *wrong_model;   // the refusal on a handle of another model
    bool names_caller;         // the wrong-model and before-reset refusals begin with "<who>: " (inherited)
    bool reset_for_all;        // every call needs the reset first; else only fleet (one refusal with the missing list: ".. come first") and
                               // fleet_state do, the world calls work before it and ask for "static_obstacles" only once it is ready (inherited)
    bool refuses_nan_entry;    // world refuses a NaN entry of the list (inherited, not designed: the other front end takes it)
    bool stores_predict;       // "predicted inside the horizon" is a flag world_vel's argument sets (a fleet switched on over a world at rest
                               // forces it to 1); else option "pf_predict", read at the time of asking
    bool tracks_with_list;     // the slot tracks are made with the first list; else with the first velocities or relayout, so that a world
                               // that never moves makes none (inherited)
    bool sep_with_front_end;   // the separation buffers come with the front end's own buffers; else with the first fleet, and fleet_state
                               // answers 1e300 / -1 from the host before that
};

constexpr WorldKind WORLD_GUIDANCE = {"guidance_", "usvmpc_guidance_world", "usvmpc_guidance_fleet", "usvmpc_guidance_reset",
                                      "the guidance front end belongs to usv_model_guidance_ca1", true, true, true, true, true, false};
constexpr WorldKind WORLD_PF = {"pf_", "usvmpc_pf_world", "usvmpc_pf_fleet", "usvmpc_pf_reset",
                                "the path-following front end (usvmpc_pf_*) belongs to usv_model_pf_ca", false, false, false, false, false, true};

// what a judge needs to know beside the world itself: which front end's call it is, and of the handle
struct WorldFacts {
    const WorldKind *kind;
    int B;
    bool model_ok;    // the handle's model is the kind's
    bool ready;       // the front end's reset has been called
    bool tracks_on;   // option "obstacle_tracks"
    bool pf_predict;  // option "pf_predict"
};

// ---- scans of a caller's array: the index of the first offending entry, n when there is none
inline size_t first_nan(const double *a, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!(a[i] == a[i])) return i;
    return n;
}

inline size_t first_nonfinite(const double *a, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (a[i] - a[i] != 0.0) return i;
    return n;
}

// Exchanged plans (fleet_plan.hpp): whether the iterate x of the handle may stand for where each vessel will go.  A mate's x[j][1] must be
// the mate's position NOW, which holds for an iterate that was solved and then handed over exactly once.  The plan hears of every event
// through a method below (no caller assigns the state); only a prepare that finds PLAN_SHIFTED launches the plan kernel, and that prepare
// uses the plan up - a second prepare without a hand-over is today's prepare.
//   PLAN_NONE     no usable plan       a front-end reset, a caller write of x (usvmpc_set, or a device pointer handed out), fleet with scene
//                                      size 0, switching plans on, a second hand-over with no solve in between, the prepare that used it
//   PLAN_SOLVED   solved, not shifted  a solve
//   PLAN_SHIFTED  one hand-over old    a hand-over (usvmpc_advance, _advance_sim, the cascade's step) from PLAN_SOLVED
enum PlanState { PLAN_NONE = 0, PLAN_SOLVED, PLAN_SHIFTED };

// the list as it stands
struct WorldState {
    bool set = false;          // a list has been given (an empty one counts)
    int nworld = 0;            // entries per instance, fleet slots included
    int nfixed = 0;            // the caller's entries (meaningful while a fleet is on)
    double max_radius = 0.0;   // (never read while nworld is 0: no entry is compared with it)
    bool moving = false;       // velocities are set for the current list
    bool predict = false;      // WorldKind::stores_predict: .. and the horizon sees them
    int fleet_S = 0;           // scene size; 0: no fleet
    double fleet_radius = 0.0;
    size_t list_cap = 0, vel_cap = 0; // doubles (vel_cap 0 with has_vel: the buffer of an empty list)
    bool has_vel = false;      // the velocity buffer exists
    bool tracks = false;       // the slot tracks exist
    bool sep = false;          // the separation buffers were made by a fleet call (WorldKind::sep_with_front_end: unused)
    bool plans = false;        // scene-mates' planned paths feed the fleet's slots (fleet_plan.hpp), when a plan is usable
    bool plan_bufs = false;    // the plan buffers (the decide step's choice, the sources, the counter) exist
    int plan = PLAN_NONE;      // PlanState: how old the iterate x is
};

enum WorldDo {
    WORLD_NOTHING = 0,
    WORLD_UPLOAD_LIST, // a fresh list of `need` doubles from the caller, into a new buffer first when `grow`
    WORLD_RELAYOUT,    // n0 entries of which f0 are fleet slots -> n1_fixed fixed entries and f1 fleet slots (fleet_relayout), with the
                       // caller's fixed entries when `new_fixed`, else the present ones; afterwards the list has velocities (`need`,
                       // `need_vel` doubles, into new buffers first when `grow`, `grow_vel`)
    WORLD_UPLOAD_VEL,  // `need` doubles of velocities from the caller, into a new buffer first when `grow`
    WORLD_MERGE_VEL,   // the caller's [B][nvel][2] into the head of every instance's [n][2]
    WORLD_STEP,        // one step over B n entries
    WORLD_READ,        // copy out B n entries; velocities from the device when `vel_on_device`, else zeros
    WORLD_FLEET_STATE, // copy out the separations; `host_answer`: no buffer yet, 1e300 / -1 from the host
    WORLD_PLANS,       // exchanged plans switched; the plan buffers first when `make_plans`
    WORLD_PLAN_STATE,  // copy out the sources and the counter; `host_answer`: no buffer yet, -1 / 0 from the host
};

// A judged call: refused (the message, word for word; nothing else is meaningful then) or what the carrier does, and the state that stands
// once it has done so.
struct WorldAct {
    std::string refused;
    WorldDo what = WORLD_NOTHING;
    size_t need = 0, need_vel = 0; // doubles (need_vel: a relayout's velocities)
    bool grow = false, grow_vel = false;
    int n0 = 0, f0 = 0, n1_fixed = 0, f1 = 0;
    bool new_fixed = false;
    int n = 0, nvel = 0;
    bool vel_on_device = false, host_answer = false;
    bool make_front_end = false; // the front end's own buffers first (a world call ahead of the reset)
    bool make_tracks = false;    // the slot tracks first
    bool make_sep = false;       // the separation buffers first, filled with 1e300 / -1
    bool make_plans = false;     // the plan buffers first: sources -1, counter 0
    bool apply_static = false;   // afterwards the carrier asks for "static_obstacles" as want_static() says
    WorldState next;
};

// The world of a handle.  Judging is const: a refused call, or one whose carrier fails, changes nothing.  Every writer is a method here; the
// handle holds one WorldPlan and assigns none of its fields.
class WorldPlan {
public:
    const WorldState &state() const { return s; }
    bool exists() const { return s.set; }
    int nworld() const { return s.nworld; }
    int nfixed() const { return s.nfixed; }
    double max_radius() const { return s.max_radius; }
    bool moving() const { return s.moving; }
    int fleet_S() const { return s.fleet_S; }
    double fleet_radius() const { return s.fleet_radius; }
    size_t list_cap() const { return s.list_cap; }
    size_t vel_cap() const { return s.vel_cap; }

    bool plans_on() const { return s.plans; }
    int plan_state() const { return s.plan; }

    // the horizon sees the velocities (only asked of a moving world)
    bool predicted(const WorldKind &k, bool pf_predict) const { return k.stores_predict ? s.predict : pf_predict; }
    bool want_static(const WorldKind &k, bool pf_predict) const { return !(s.moving && predicted(k, pf_predict)); }
    // a prepare: its decide step records the choice (plans on over a fleet that is predicted) .. and the plan kernel follows it
    bool records_choice(const WorldKind &k, bool pf_predict) const { return s.plans && s.fleet_S != 0 && !want_static(k, pf_predict); }
    bool plan_usable(const WorldKind &k, bool pf_predict) const { return records_choice(k, pf_predict) && s.plan == PLAN_SHIFTED; }
    // what happens to the iterate x (PlanState above)
    void plan_solved() { s.plan = PLAN_SOLVED; }
    void plan_handed_over() { s.plan = s.plan == PLAN_SOLVED ? PLAN_SHIFTED : PLAN_NONE; }
    void plan_lost() { s.plan = PLAN_NONE; } // (a front-end reset, a caller write of x)
    void plan_used() { s.plan = PLAN_NONE; } // (the prepare that launched the plan kernel)
    // usvmpc_advance / _advance_sim / the cascade's hand-over move the world on
    bool steps_on_advance(bool step_on_advance) const { return s.moving && step_on_advance; }

    WorldAct world(const WorldFacts &f, const double *list, int n_world, double max_radius) const
    {
        const WorldKind &k = *f.kind;
        const std::string who = std::string(k.prefix) + "world";
        WorldAct a = begin(f, who, k.reset_for_all);
        if (!a.refused.empty()) return a;
        if (n_world < 0 || n_world > WORLD_LMAX) return refuse(who + ": n_world must lie in 0.." + std::to_string(WORLD_LMAX));
        if (n_world > 0 && !list) return refuse(who + ": null world list");
        if (!(max_radius == max_radius)) return refuse(who + ": max_radius is NaN");
        const size_t need = (size_t)f.B * (size_t)n_world * 3;
        if (k.refuses_nan_entry) {
            const size_t i = first_nan(list, need);
            if (i < need) return refuse(who + ": entry " + std::to_string(i) + " is NaN");
        }
        a.next.max_radius = max_radius;
        if (s.fleet_S) { // (the fixed entries only; the fleet slots stay)
            const int f0 = fleet_slots(s.fleet_S);
            if (!fleet_fits(n_world, s.fleet_S))
                return refuse(who + ": a fleet is on and owns " + std::to_string(f0) + " entries of the list: n_world must lie in 0.." +
                              std::to_string(WORLD_LMAX - f0));
            relayout(a, f, n_world, f0, true);
            a.next.nfixed = n_world;
            return a;
        }
        a.what = WORLD_UPLOAD_LIST;
        a.need = need;
        a.grow = need > s.list_cap;
        a.make_front_end = !k.reset_for_all;
        a.make_tracks = k.tracks_with_list && !s.tracks;
        a.next.tracks = s.tracks || a.make_tracks;
        const bool same = s.set && s.nworld == n_world;
        a.next.set = true;
        a.next.nworld = n_world;
        if (s.moving && !same) { // (velocities belong to a list: another n_world is at rest until its own are given)
            a.next.moving = false;
            a.apply_static = f.ready;
        }
        return a;
    }

    WorldAct vel(const WorldFacts &f, const double *v, int predict) const
    {
        const WorldKind &k = *f.kind;
        const std::string who = std::string(k.prefix) + "world_vel";
        WorldAct a = begin(f, who, k.reset_for_all);
        if (!a.refused.empty()) return a;
        if (!v) { // back to a world at rest
            if (s.fleet_S) return refuse(who + ": a fleet is on and its world moves; switch it off first (" + k.fleet_call + " with scene_size 0)");
            a.next.moving = false;
            a.apply_static = f.ready;
            return a;
        }
        if (!s.set) return refuse(who + ": no world list yet (" + k.world_call + " first)");
        if (f.tracks_on) return refuse(who + ": option \"obstacle_tracks\" is on and the tracks own p; switch it off first");
        a.nvel = s.fleet_S ? s.nfixed : s.nworld; // (a fleet's slots have the velocities the gather gave them)
        a.need = (size_t)f.B * (size_t)a.nvel * 2;
        const size_t i = first_nonfinite(v, a.need);
        if (i < a.need) return refuse(who + ": entry " + std::to_string(i) + " is not finite");
        a.n = s.nworld;
        if (k.stores_predict) a.next.predict = predict != 0;
        // (the path-following copy did not ask for "static_obstacles" after a merge: the guarded request is a no-op there, the world moves
        // already and option "pf_predict" has its own hook)
        a.apply_static = f.ready;
        if (s.fleet_S) {
            a.what = WORLD_MERGE_VEL;
            return a;
        }
        a.what = WORLD_UPLOAD_VEL;
        a.grow = a.need > s.vel_cap || !s.has_vel; // (an empty list moves too: the buffer's existence is what tells a prepare so)
        a.make_tracks = !s.tracks; // (WorldKind::tracks_with_list: they exist since the list)
        a.next.tracks = true;
        a.next.moving = true;
        return a;
    }

    WorldAct step(const WorldFacts &f, double T) const
    {
        const WorldKind &k = *f.kind;
        const std::string who = std::string(k.prefix) + "world_step";
        WorldAct a = begin(f, who, k.reset_for_all);
        if (!a.refused.empty()) return a;
        if (!s.moving) return refuse(who + ": the world is at rest (" + k.world_call + "_vel first)");
        if (T - T != 0.0) return refuse(who + ": T is not finite");
        a.what = s.nworld ? WORLD_STEP : WORLD_NOTHING;
        a.n = s.nworld;
        return a;
    }

    WorldAct read(const WorldFacts &f) const
    {
        const WorldKind &k = *f.kind;
        const std::string who = std::string(k.prefix) + "world_read";
        WorldAct a = begin(f, who, k.reset_for_all);
        if (!a.refused.empty()) return a;
        if (!s.set) return refuse(who + ": no world list yet (" + k.world_call + " first)");
        a.what = WORLD_READ;
        a.n = s.nworld;
        a.vel_on_device = s.moving;
        return a;
    }

    WorldAct fleet(const WorldFacts &f, int scene_size, double radius) const
    {
        const WorldKind &k = *f.kind;
        const std::string who = std::string(k.prefix) + "fleet";
        WorldAct a = begin(f, who, k.reset_for_all);
        if (!a.refused.empty()) return a;
        if (k.reset_for_all) {
            if (!s.set) return refuse(who + ": no world list yet (" + k.world_call + " first; an empty one will do)");
        } else if (!f.ready || !s.set)
            return refuse(who + ": " + k.reset_call + " and a world list (" + k.world_call + "; an empty one will do) come first");
        if (scene_size < 0) return refuse(who + ": scene_size must not be negative");
        if (!fleet_on(scene_size)) { // off: the list is cut back to the fixed entries, which keep their velocities
            a.next.plan = PLAN_NONE;
            if (!s.fleet_S) return a;
            relayout(a, f, s.nfixed, 0, false);
            a.next.fleet_S = 0;
            return a;
        }
        const int n_fixed = s.fleet_S ? s.nfixed : s.nworld;
        if (f.tracks_on) return refuse(who + ": option \"obstacle_tracks\" is on and the tracks own p; switch it off first");
        if (!fleet_scene_ok(f.B, scene_size))
            return refuse(who + ": the batch of " + std::to_string(f.B) + " is not a whole number of scenes of " + std::to_string(scene_size));
        if (!fleet_fits(n_fixed, scene_size))
            return refuse(who + ": " + std::to_string(n_fixed) + " fixed entries and " + std::to_string(scene_size - 1) + " fleet entries exceed the " +
                          std::to_string(WORLD_LMAX) + " of a world list");
        if (!fleet_radius_ok(radius)) return refuse(who + ": radius must be finite and not negative");
        relayout(a, f, n_fixed, scene_size - 1, false);
        a.make_sep = !k.sep_with_front_end && !s.sep;
        a.next.sep = s.sep || a.make_sep;
        if (k.stores_predict && !s.moving) a.next.predict = true; // (a world at rest had no say in it; world_vel changes it)
        a.next.fleet_S = scene_size;
        a.next.nfixed = n_fixed;
        a.next.fleet_radius = radius;
        a.next.moving = true;
        a.apply_static = true;
        return a;
    }

    WorldAct fleet_state(const WorldFacts &f) const
    {
        const WorldKind &k = *f.kind;
        WorldAct a = begin(f, std::string(k.prefix) + "fleet_state", true);
        if (!a.refused.empty()) return a;
        a.what = WORLD_FLEET_STATE;
        a.host_answer = !k.sep_with_front_end && !s.sep; // no fleet yet: as after a reset
        return a;
    }

    // exchanged plans on or off (N: the handle's horizon)
    WorldAct plans(const WorldFacts &f, int on, int N) const
    {
        const WorldKind &k = *f.kind;
        const std::string who = std::string(k.prefix) + "fleet_plans";
        WorldAct a = begin(f, who, k.reset_for_all);
        if (!a.refused.empty()) return a;
        if (k.reset_for_all) {
            if (!s.fleet_S) return refuse(who + ": a world list and a fleet (" + k.fleet_call + ") come first");
        } else if (!f.ready || !s.fleet_S)
            return refuse(who + ": " + k.reset_call + ", a world list and a fleet (" + k.fleet_call + ") come first");
        if (N < 2) return refuse(who + ": the horizon has N = " + std::to_string(N) + "; a scene-mate's plan needs N >= 2");
        a.what = WORLD_PLANS;
        a.make_plans = on != 0 && !s.plan_bufs;
        a.next.plans = on != 0;
        if (on) { // (whatever the iterate was: the first plan used is one solved and handed over with plans on)
            a.next.plan_bufs = true;
            a.next.plan = PLAN_NONE;
        }
        return a;
    }

    WorldAct fleet_plan_state(const WorldFacts &f) const
    {
        const WorldKind &k = *f.kind;
        WorldAct a = begin(f, std::string(k.prefix) + "fleet_plan_state", true);
        if (!a.refused.empty()) return a;
        a.what = WORLD_PLAN_STATE;
        a.host_answer = !s.plan_bufs; // plans were never on
        return a;
    }

    // the carrier has done what `a` says
    void commit(const WorldAct &a)
    {
        const WorldState was = s;
        s = a.next;
        s.list_cap = was.list_cap; s.vel_cap = was.vel_cap; s.has_vel = was.has_vel; // (the buffers' own facts, below)
    }
    // the carrier has released a buffer (0, false) or made a new one: the buffers' own facts, which stand even when the call then fails
    void list_buffer(size_t cap) { s.list_cap = cap; }
    void vel_buffer(size_t cap, bool exists) { s.vel_cap = cap; s.has_vel = exists; }

private:
    WorldState s;

    static WorldAct refuse(const std::string &why)
    {
        WorldAct a;
        a.refused = why;
        return a;
    }

    // the refusals every call begins with; else an act that does nothing and leaves the state as it is
    WorldAct begin(const WorldFacts &f, const std::string &who, bool need_ready) const
    {
        const WorldKind &k = *f.kind;
        const std::string lead = k.names_caller ? who + ": " : std::string();
        if (!f.model_ok) return refuse(lead + k.wrong_model);
        if (need_ready && !f.ready) return refuse(lead + k.reset_call + " must be called first");
        WorldAct a;
        a.next = s;
        return a;
    }

    // the present list -> n1_fixed fixed entries and f1 fleet slots
    void relayout(WorldAct &a, const WorldFacts &f, int n1_fixed, int f1, bool new_fixed) const
    {
        a.what = WORLD_RELAYOUT;
        a.n0 = s.nworld; a.f0 = fleet_slots(s.fleet_S); a.n1_fixed = n1_fixed; a.f1 = f1;
        a.new_fixed = new_fixed;
        a.need = (size_t)f.B * (size_t)(n1_fixed + f1) * 3;
        a.grow = a.need > s.list_cap;
        a.need_vel = (size_t)f.B * (size_t)(n1_fixed + f1) * 2;
        a.grow_vel = a.need_vel > s.vel_cap || !s.has_vel;
        a.make_tracks = !s.tracks; // (WorldKind::tracks_with_list: they exist since the list)
        a.next.tracks = true;
        a.next.nworld = n1_fixed + f1;
    }
};

} // namespace usv
