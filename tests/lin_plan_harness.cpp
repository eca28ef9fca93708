// The lineariser's schedule (csrc/lin_plan.hpp) on the host: a handle made of numbers, driven from the command line.
// Arguments, in order: name=value sets an input of the next solves (hand: whether their QP launch hands instances over - what launch_qp
// reports; map: the map DevPtrs::perm names, 0 none / 1 buffer A / 2 buffer B, for what usvmpc_set_option does to it); "solve" runs plan_lin
// on what is set and prints one line - the plan, then (as launch_solve does after its QP launch) launched_ahead when the plan says so, the
// mode and grid of that pass, and the schedule's state afterwards; "write", "cancel" (prints whether to synchronise) and "sync" are
// LinSched's caller_wrote, cancel and synced; "grid" prints count / blocks / block of every mode for N, Bp, unpaired and paired.
// Schedule, solve number and running map persist from one token to the next, as in a handle.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "lin_plan.hpp"

using namespace usv;

static void print_launch(const char *name, const LinLaunch &l) { printf(" %s=%d:%ld:%d:%ld", name, l.mode, l.blocks, l.block, l.count); }

int main(int argc, char **argv)
{
    LinIn in = {};
    // a handle as usvmpc_create leaves it: no mirror (a large batch), sorting on, the paired lineariser
    in.phase = 0; in.nsolves = 0; in.B = 16384; in.Bp = -1; in.N = 20;
    in.pipeline = true; in.dynamic_rows = true; in.sort_enabled = true; in.sort_two = false; in.lin_force = 0; in.pairs = true; in.cond = false;
    in.mirror = false; in.extern_access = false; in.cur_map = MAP_NONE;
    LinSched s;
    s.reset();
    bool hand = false;
    int Bp_set = -1;
    for (int a = 1; a < argc; a++) {
        const std::string arg = argv[a];
        in.Bp = Bp_set >= 0 ? Bp_set : (in.B + 3) / 4 * 4; // (the handle pads the batch to the QP kernel's four rows)
        if (arg == "write") { s.caller_wrote(); continue; }
        if (arg == "sync") { s.synced(); continue; }
        if (arg == "cancel") { printf("cancel sync=%d\n", (int)s.cancel()); continue; }
        if (arg == "grid") {
            for (int pairs = 0; pairs < 2; pairs++)
                for (int mode = 0; mode < LIN_MODES; mode++) {
                    const LinLaunch l = lin_launch(mode, pairs != 0, in.N, in.Bp);
                    printf("grid pairs=%d mode=%d count=%ld blocks=%ld block=%d lin_block=%d\n", pairs, l.mode, l.count, l.blocks, l.block, lin_block(mode));
                }
            printf("redo_words=%d\n", redo_words(in.N));
            continue;
        }
        if (arg == "solve") {
            const LinPlan p = plan_lin(in, s);
            printf("pipe=%d wait=%d use=%d map_from=%s map=%d map_changed=%d spec_next=%d redo=%d clear_redo=%d nlaunch=%d", (int)p.pipe, (int)p.wait_ahead,
                   (int)p.use_ahead, p.map_from == LinPlan::KEEP ? "keep" : p.map_from == LinPlan::AHEAD ? "ahead" : "sort", (int)p.map, (int)p.map_changed,
                   (int)p.spec_next, (int)p.redo, (int)p.clear_redo, p.nlaunch);
            print_launch("l0", p.launch[0]);
            if (p.nlaunch > 1) print_launch("l1", p.launch[1]);
            printf(" forced=%d force_epoch=%d pair_launches=%d sort_next=%d next_map=%d copy_iter_prev=%d", (int)p.forced, p.forced ? p.force_epoch : 0,
                   p.pair_launches, (int)p.sort_next, (int)p.next_map, (int)p.copy_iter_prev);
            in.cur_map = p.map;
            int ahead = -1;
            if (p.spec_next) {
                ahead = s.launched_ahead(hand, p.next_map);
                print_launch("la", lin_launch(ahead, in.pairs, in.N, in.Bp));
            }
            printf(" ahead=%d made_for=%ld valid=%d outstanding=%d quiet=%d smap=%d fine=%d hits=%ld misses=%ld\n", ahead, s.made_for, (int)s.valid,
                   (int)s.outstanding, s.quiet, (int)s.map, (int)s.fine, s.hits, s.misses);
            in.nsolves++;
            continue;
        }
        const size_t eq = arg.find('=');
        if (eq == std::string::npos) { fprintf(stderr, "bad argument '%s'\n", argv[a]); return 2; }
        const std::string key = arg.substr(0, eq);
        const long v = atol(arg.c_str() + eq + 1);
        if (key == "phase") in.phase = (int)v;
        else if (key == "B") in.B = (int)v;
        else if (key == "Bp") Bp_set = (int)v;
        else if (key == "N") in.N = (int)v;
        else if (key == "pipeline") in.pipeline = v != 0;
        else if (key == "dynamic_rows") in.dynamic_rows = v != 0;
        else if (key == "sort") in.sort_enabled = v != 0;
        else if (key == "sort_two") in.sort_two = v != 0;
        else if (key == "lin_force") in.lin_force = (int)v;
        else if (key == "pairs") in.pairs = v != 0;
        else if (key == "cond") in.cond = v != 0;
        else if (key == "mirror") in.mirror = v != 0;
        else if (key == "extern") in.extern_access = v != 0;
        else if (key == "map") in.cur_map = (LinMap)v;
        else if (key == "hand") hand = v != 0;
        else { fprintf(stderr, "unknown name '%s'\n", key.c_str()); return 2; }
    }
    return 0;
}
