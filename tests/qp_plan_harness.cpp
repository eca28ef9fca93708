// The QP launch policy (csrc/qp_plan.hpp) on the host, against a device made of numbers: 256 CUs, and a CU holds
//     min(max_<slot>, 160 KB / (st_<slot> + dynamic bytes))
// workgroups of a kernel, whatever their size (max_<slot>, st_<slot>: the slot's ceiling and static LDS, from the command line).
// Arguments, in order: name=value sets an input, a table fact or a figure of the device; "plan" runs plan_qp on what is set and prints
// one line - the plan, the caps afterwards, the probe calls that plan made (slot:block:bytes, or static:slot); "reset" is QpCaps::reset().
// The caps persist from one "plan" to the next, as in a handle.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "qp_plan.hpp"

using namespace usv;

static const char *const SLOT_NAMES[SLOT_COUNT] = {"qp", "qp_lds", "qp_aux", "wide_lds1", "wide_hbm1", "wide_lds4", "wide_hbm4", "resume", "resume_lds"};

struct FakeDevice {
    long max_wgs[SLOT_COUNT], st[SLOT_COUNT];
    std::string calls;
    int blocks(QpSlot s, int block, size_t dyn)
    {
        calls += std::string(calls.empty() ? "" : ",") + SLOT_NAMES[s] + ":" + std::to_string(block) + ":" + std::to_string(dyn);
        const long bytes = st[s] + (long)dyn;
        return (int)(bytes > 0 ? std::min(max_wgs[s], CU_LDS_BYTES / bytes) : max_wgs[s]);
    }
    long static_lds(QpSlot s)
    {
        calls += std::string(calls.empty() ? "" : ",") + "static:" + SLOT_NAMES[s];
        return st[s];
    }
};

int main(int argc, char **argv)
{
    QpIn in = {};
    // a handle as usvmpc_create leaves it, over a table that has every kernel
    in.B = 1; in.Bp = -1; in.N = 20; in.K = 3; in.npt = 36; in.nu = 2; in.aux_dense4 = 4; in.kch = 1; in.phase = 0; in.ncu = 256;
    in.wide_mode = -1; in.wide_waves = -1; in.lds_mode = -1; in.dynamic_rows = true; in.max_waves = 0; in.aux_lds = true;
    in.handover_iter = -1; in.handover_lds = true; in.handover_co = -1; in.co_wgs = 0; in.own_stream = true;
    for (bool &e : in.has) e = true;
    in.has_resume_co = true;
    in.nplw = 28; in.ex_lds = 6; in.ex_hbm = 10; in.k_kch = 1; in.k_soft = false;
    FakeDevice dev;
    for (int s = 0; s < SLOT_COUNT; s++) { dev.max_wgs[s] = 8; dev.st[s] = 0; }
    QpCaps caps;
    caps.reset();
    int Bp_set = -1;
    for (int a = 1; a < argc; a++) {
        const std::string arg = argv[a];
        if (arg == "reset") { caps.reset(); continue; }
        if (arg == "plan") {
            in.Bp = Bp_set >= 0 ? Bp_set : (in.B + 3) / 4 * 4; // (the handle pads the batch to the QP kernel's four rows)
            dev.calls.clear();
            const QpPlan p = plan_qp(in, caps, dev);
            printf("slot=%s grid=%ld block=%d lds=%zu ngroups=%ld q0=%d rows=%d mapping=%d hand_ready=%d hand=%d hand_lds=%d hand_bytes=%zu hand_iter=%d hand_wgs=%ld co=%d co_wgs=%ld",
                   SLOT_NAMES[p.slot], p.grid, p.block, p.lds_bytes, p.ngroups, p.q0, p.rows, p.mapping, (int)p.hand_ready, (int)p.hand, (int)p.hand_lds,
                   p.hand ? p.hand_bytes : (size_t)0, p.hand_iter, p.hand ? p.hand_wgs : 0L, (int)p.co, p.co_wgs);
            printf(" cap_qp=%ld cap_lds=%ld cap_aux=%ld cap_wide=%ld cap_wide_hbm=%ld cap_wide4=%ld cap_wide4_hbm=%ld cap_resume=%ld cap_resume_lds=%d cap_lds_static=%ld",
                   caps.qp, caps.lds, caps.aux, caps.wide, caps.wide_hbm, caps.wide4, caps.wide4_hbm, caps.resume, (int)caps.resume_lds, caps.lds_static);
            printf(" probes=%s\n", dev.calls.c_str());
            continue;
        }
        const size_t eq = arg.find('=');
        if (eq == std::string::npos) { fprintf(stderr, "bad argument '%s'\n", argv[a]); return 2; }
        const std::string key = arg.substr(0, eq);
        const long v = atol(arg.c_str() + eq + 1);
        bool known = true;
        if (key == "B") in.B = (int)v;
        else if (key == "Bp") Bp_set = (int)v;
        else if (key == "N") in.N = (int)v;
        else if (key == "K") in.K = (int)v;
        else if (key == "npt") in.npt = (int)v;
        else if (key == "nu") in.nu = (int)v;
        else if (key == "aux_dense4") in.aux_dense4 = (int)v;
        else if (key == "kch") in.kch = (int)v;
        else if (key == "phase") in.phase = (int)v;
        else if (key == "ncu") in.ncu = (int)v;
        else if (key == "wide") in.wide_mode = (int)v;
        else if (key == "wide_waves") in.wide_waves = (int)v;
        else if (key == "lds_workspace") in.lds_mode = (int)v;
        else if (key == "dynamic_rows") in.dynamic_rows = v != 0;
        else if (key == "max_waves") in.max_waves = v;
        else if (key == "aux_in_lds") in.aux_lds = v != 0;
        else if (key == "handover_iter") in.handover_iter = (int)v;
        else if (key == "handover_lds") in.handover_lds = v != 0;
        else if (key == "handover_co") in.handover_co = (int)v;
        else if (key == "co_wgs") in.co_wgs = v;
        else if (key == "own_stream") in.own_stream = v != 0;
        else if (key == "has_resume_co") in.has_resume_co = v != 0;
        else if (key == "nplw") in.nplw = (int)v;
        else if (key == "ex_lds") in.ex_lds = (int)v;
        else if (key == "ex_hbm") in.ex_hbm = (int)v;
        else if (key == "k_kch") in.k_kch = (int)v;
        else if (key == "k_soft") in.k_soft = v != 0;
        else {
            known = false;
            for (int s = 0; s < SLOT_COUNT && !known; s++) {
                known = true;
                if (key == std::string("has_") + SLOT_NAMES[s]) in.has[s] = v != 0;
                else if (key == std::string("max_") + SLOT_NAMES[s]) dev.max_wgs[s] = v;
                else if (key == std::string("st_") + SLOT_NAMES[s]) dev.st[s] = v;
                else known = false;
            }
        }
        if (!known) { fprintf(stderr, "unknown name '%s'\n", key.c_str()); return 2; }
    }
    return 0;
}
