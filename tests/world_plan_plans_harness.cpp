// Command-line driver of csrc/world_plan.hpp for exchanged plans (tests/test_world_plan_plans.py; beside world_plan_harness.cpp, which
// drives the list itself): the judge `plans`, the three-state member PlanState and the events that move it, compiled with the host compiler
// only.  The carrier is played here: a judged call that is not refused is committed; a prepare launches the plan kernel exactly when
// plan_usable() says so, and then uses the plan up, as usvmpc.hip's fleet_plans_follow does.
// Tokens, left to right:
//   kind:g | kind:p                     the front end (guidance: default)
//   B:n  N:n  model:0|1  ready:0|1  pfpredict:0|1        the facts a judge is given (defaults 6, 6, 1, 1, 1)
//   commit:0|1                          0: judged calls are not committed - a carrier that failed (default 1)
//   world:n  fleet:S  vel:predict       the list's own calls (radius 0.5; vel: velocities for the fixed entries, with `predict`)
//   plans:on  pstate                    usvmpc_*_fleet_plans, usvmpc_*_fleet_plan_state
//   solve  advance  setx  reset  prepare                 the events: a solve, a hand-over, a caller write of x, the front end's reset,
//                                       a device-resident prepare
//   state                               no call: the state line alone
// Every judged call prints "<call> rc=-1 err=<text>" or "<call> rc=0 what= make_plans= host_answer=", every event "<event> launched=0|1"
// (launched: a prepare launched the plan kernel), and then the state: "state plans= plan= plan_bufs= fleet_S= nworld= records= usable=
// launches=".
#include "world_plan.hpp"

#include <cstdio>
#include <cstdlib>
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

int main(int argc, char **argv)
{
    WorldFacts f = {&WORLD_GUIDANCE, 6, true, true, false, true};
    int N = 6;
    bool commit = true;
    long launches = 0;
    WorldPlan plan;
    for (int a = 1; a < argc; a++) {
        const std::vector<std::string> w = split(argv[a]);
        auto num = [&](size_t j) { return j < w.size() ? (int)std::strtol(w[j].c_str(), nullptr, 0) : 0; };
        WorldAct act;
        bool judged = true;
        if (w[0] == "kind") { f.kind = w.size() > 1 && w[1] == "p" ? &WORLD_PF : &WORLD_GUIDANCE; continue; }
        else if (w[0] == "B") { f.B = num(1); continue; }
        else if (w[0] == "N") { N = num(1); continue; }
        else if (w[0] == "model") { f.model_ok = num(1) != 0; continue; }
        else if (w[0] == "ready") { f.ready = num(1) != 0; continue; }
        else if (w[0] == "pfpredict") { f.pf_predict = num(1) != 0; continue; }
        else if (w[0] == "commit") { commit = num(1) != 0; continue; }
        else if (w[0] == "world") {
            const int n = num(1);
            std::vector<double> list((size_t)f.B * (size_t)(n > 0 ? n : 0) * 3, 1.0);
            act = plan.world(f, list.empty() ? nullptr : list.data(), n, 100.0);
        } else if (w[0] == "vel") {
            const int nvel = plan.fleet_S() ? plan.nfixed() : plan.nworld();
            std::vector<double> v((size_t)f.B * (size_t)nvel * 2 + 1, 0.125);
            act = plan.vel(f, v.data(), num(1));
        } else if (w[0] == "fleet") act = plan.fleet(f, num(1), 0.5);
        else if (w[0] == "plans") act = plan.plans(f, num(1), N);
        else if (w[0] == "pstate") act = plan.fleet_plan_state(f);
        else {
            judged = false;
            bool launched = false;
            if (w[0] == "solve") plan.plan_solved();
            else if (w[0] == "advance") plan.plan_handed_over();
            else if (w[0] == "setx" || w[0] == "reset") plan.plan_lost();
            else if (w[0] == "prepare") {
                launched = plan.plan_usable(*f.kind, f.pf_predict);
                if (launched) { launches++; plan.plan_used(); }
            } else if (w[0] != "state") { std::printf("bad token %s\n", argv[a]); return 2; }
            if (w[0] != "state") std::printf("%s launched=%d\n", w[0].c_str(), (int)launched);
        }
        if (judged) {
            if (!act.refused.empty()) std::printf("%s rc=-1 err=%s\n", w[0].c_str(), act.refused.c_str());
            else {
                std::printf("%s rc=0 what=%d make_plans=%d host_answer=%d\n", w[0].c_str(), (int)act.what, (int)act.make_plans, (int)act.host_answer);
                if (commit) {
                    if (act.grow) { if (act.what == WORLD_UPLOAD_VEL) plan.vel_buffer(act.need, true); else plan.list_buffer(act.need); }
                    if (act.grow_vel) plan.vel_buffer(act.need_vel, true);
                    plan.commit(act);
                }
            }
        }
        const WorldState &s = plan.state();
        std::printf("state plans=%d plan=%d plan_bufs=%d fleet_S=%d nworld=%d records=%d usable=%d launches=%ld\n", (int)s.plans, s.plan,
                    (int)s.plan_bufs, s.fleet_S, s.nworld, (int)plan.records_choice(*f.kind, f.pf_predict), (int)plan.plan_usable(*f.kind, f.pf_predict),
                    launches);
    }
    return 0;
}
