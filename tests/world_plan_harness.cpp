// Command-line driver of csrc/world_plan.hpp (tests/test_world_plan.py): the front ends' resident world list - what a call refuses, what the
// carrier is told to do and what the list is afterwards - compiled with the host compiler only.  The carrier is played here: a judged call
// that is not refused is committed, and a buffer the act says is to be replaced is reported to the plan as usvmpc.hip's world_buffer does.
// Tokens, left to right:
//   kind:g | kind:p                     the front end (guidance: default)
//   B:n  model:0|1  ready:0|1  tracks:0|1  pfpredict:0|1      the facts a judge is given (defaults 6, 1, 1, 0, 1)
//   commit:0|1                          0: judged calls are not committed (default 1)
//   world:n:radius[:null | :nan=i]      a list of n entries per instance, entry j of the array = j (null: no array; nan=i: entry i is NaN)
//   vel:null:predict | vel:predict[:nan=i | :inf=i]           velocities for the list as it stands, entry j = j / 8
//   fleet:S:radius   step:T   read   fstate                   (radius, T: strtod, "nan" and "inf" included)
//   state                               no call: the state line alone
// Every call prints one line, "<call> rc=-1 err=<text>" or "<call> rc=0 what= need= grow= need_vel= grow_vel= n0= f0= n1_fixed= f1=
// new_fixed= n= nvel= vel_on_device= host_answer= make_front_end= make_tracks= make_sep= apply_static=", and then the plan's state,
// "state set= nworld= nfixed= max_radius= moving= predict= fleet_S= fleet_radius= list_cap= vel_cap= has_vel= tracks= sep= predicted=
// want_static= steps=".
#include "world_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

using namespace usv;

static std::vector<std::string> split(const std::string &s)
{
    std::vector<std::string> out;
    size_t a = 0;
    for (;;) {
        const size_t b = s.find(':', a);
        out.push_back(s.substr(a, b == std::string::npos ? b : b - a));
        if (b == std::string::npos) return out;
        a = b + 1;
    }
}

// "nan=7" / "inf=7": entry 7 of v becomes that
static void spoil(std::vector<double> &v, const std::string &w)
{
    const size_t eq = w.find('=');
    if (eq == std::string::npos) return;
    const size_t i = (size_t)std::strtoull(w.c_str() + eq + 1, nullptr, 0);
    if (i < v.size()) v[i] = w.compare(0, 3, "nan") == 0 ? std::numeric_limits<double>::quiet_NaN() : std::numeric_limits<double>::infinity();
}

int main(int argc, char **argv)
{
    WorldFacts f = {&WORLD_GUIDANCE, 6, true, true, false, true};
    bool commit = true;
    WorldPlan plan;
    for (int a = 1; a < argc; a++) {
        const std::vector<std::string> w = split(argv[a]);
        auto num = [&](size_t j) { return j < w.size() ? (int)std::strtol(w[j].c_str(), nullptr, 0) : 0; };
        auto real = [&](size_t j) { return j < w.size() ? std::strtod(w[j].c_str(), nullptr) : 0.0; };
        WorldAct act;
        if (w[0] == "kind") { f.kind = w.size() > 1 && w[1] == "p" ? &WORLD_PF : &WORLD_GUIDANCE; continue; }
        else if (w[0] == "B") { f.B = num(1); continue; }
        else if (w[0] == "model") { f.model_ok = num(1) != 0; continue; }
        else if (w[0] == "ready") { f.ready = num(1) != 0; continue; }
        else if (w[0] == "tracks") { f.tracks_on = num(1) != 0; continue; }
        else if (w[0] == "pfpredict") { f.pf_predict = num(1) != 0; continue; }
        else if (w[0] == "commit") { commit = num(1) != 0; continue; }
        else if (w[0] == "world") {
            const int n = num(1);
            std::vector<double> list(n > 0 && n <= 4096 ? (size_t)f.B * (size_t)n * 3 : 0);
            for (size_t j = 0; j < list.size(); j++) list[j] = (double)j;
            const bool null = w.size() > 3 && w[3] == "null";
            if (w.size() > 3) spoil(list, w[3]);
            act = plan.world(f, null || list.empty() ? nullptr : list.data(), n, real(2));
        } else if (w[0] == "vel") {
            const bool null = w.size() > 1 && w[1] == "null";
            const int nvel = plan.fleet_S() ? plan.nfixed() : plan.nworld();
            std::vector<double> v((size_t)f.B * (size_t)nvel * 2 + 1); // (+ 1: an empty list's velocities are still an array)
            for (size_t j = 0; j < v.size(); j++) v[j] = (double)j / 8.0;
            if (!null && w.size() > 2) spoil(v, w[2]);
            act = plan.vel(f, null ? nullptr : v.data(), null ? num(2) : num(1));
        } else if (w[0] == "fleet") act = plan.fleet(f, num(1), real(2));
        else if (w[0] == "step") act = plan.step(f, real(1));
        else if (w[0] == "read") act = plan.read(f);
        else if (w[0] == "fstate") act = plan.fleet_state(f);
        else if (w[0] != "state") { std::printf("bad token %s\n", argv[a]); return 2; }
        if (w[0] == "state") {} // (the state line alone)
        else if (!act.refused.empty()) std::printf("%s rc=-1 err=%s\n", w[0].c_str(), act.refused.c_str());
        else {
            std::printf("%s rc=0 what=%d need=%zu grow=%d need_vel=%zu grow_vel=%d n0=%d f0=%d n1_fixed=%d f1=%d new_fixed=%d n=%d nvel=%d "
                        "vel_on_device=%d host_answer=%d make_front_end=%d make_tracks=%d make_sep=%d apply_static=%d\n",
                        w[0].c_str(), (int)act.what, act.need, (int)act.grow, act.need_vel, (int)act.grow_vel, act.n0, act.f0, act.n1_fixed, act.f1,
                        (int)act.new_fixed, act.n, act.nvel, (int)act.vel_on_device, (int)act.host_answer, (int)act.make_front_end,
                        (int)act.make_tracks, (int)act.make_sep, (int)act.apply_static);
            if (commit) {
                const bool vel = act.what == WORLD_UPLOAD_VEL;
                if (act.grow) { if (vel) plan.vel_buffer(act.need, true); else plan.list_buffer(act.need); }
                if (act.grow_vel) plan.vel_buffer(act.need_vel, true);
                plan.commit(act);
            }
        }
        const WorldState &s = plan.state();
        std::printf("state set=%d nworld=%d nfixed=%d max_radius=%g moving=%d predict=%d fleet_S=%d fleet_radius=%g list_cap=%zu vel_cap=%zu has_vel=%d "
                    "tracks=%d sep=%d predicted=%d want_static=%d steps=%d\n",
                    (int)s.set, s.nworld, s.nfixed, s.max_radius, (int)s.moving, (int)s.predict, s.fleet_S, s.fleet_radius, s.list_cap, s.vel_cap,
                    (int)s.has_vel, (int)s.tracks, (int)s.sep, (int)plan.predicted(*f.kind, f.pf_predict), (int)plan.want_static(*f.kind, f.pf_predict),
                    (int)plan.steps_on_advance(true));
    }
    return 0;
}
