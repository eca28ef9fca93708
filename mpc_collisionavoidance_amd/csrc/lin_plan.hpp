// lin_plan.hpp — when the lineariser runs, under which group -> instance map and over which grid: the schedule of the pipelined lineariser
// as a host-only state machine (LinSched) and a pure function from numbers (the handle's sizes and options, the solve's number and phase)
// to what one solve does ahead of its QP launch (plan_lin).  No HIP header and no pointer: usvmpc.hip's launch_solve fills LinIn, carries the
// plan out and reports the QP launch's hand-over back (launched_ahead); tests/lin_plan_harness.cpp drives the same code from a command line.
//
// Pipelined lineariser (option "pipeline_linearize"): the lineariser of tick t + 1 is launched on a second stream right behind the
// QP launch of tick t; its workgroups are dispatched as that launch's persistent waves leave, i.e. it runs in the launch's tail
// (profiles/r03_tail.txt: the last ~14 ms of a 76 ms launch run on a device that is being vacated).  An instance is linearised
// there only when its own results AND those of the instance still owning the target planes are final (DevPtrs::epoch); the few
// that were not are redone by a fix-up pass in front of the next QP launch.  The queue order of a tick is then fixed one tick
// earlier (from the counts of two solves back).  Scheduling only: results are bit-identical.
#pragma once

#include "lin_order.hpp"

namespace usv {

// usv_linearize MODE: 0 the whole batch; 1 / 3 speculative for the next tick beside a running QP launch; 2 / 4 fix-up of what that pass
// skipped (linearize.hpp; the workgroups of each: usvmpc.hip, usv_linearize)
constexpr int LIN_MODES = 5;
constexpr int LIN_GROUP_LANES = 16;        // lanes of a group (params.hpp LANES)
constexpr int LIN_WAVE = 64;
// The pipeline pays from this batch size on (RTI solves only; bench.py states the same figure for its workloads)
constexpr int PIPELINE_MIN_BATCH = 16384;
// The lineariser runs ahead only from this many quiet RTI solves in a row on (LinSched::quiet) - a caller that sets yref / x / u every tick (the
// reference's protocol: scripts/usv_guidance_ca1/main.py:123-130) never pays for a speculative pass that is thrown away
constexpr int SPEC_QUIET_MIN = 2;

// ---- grids (usv_linearize): threads of a workgroup, what `n` counts, workgroups
constexpr int lin_block(int mode) { return mode == 3 ? LIN_WAVE : 256; }
// (group, stage) pairs - or work items -, groups for MODE 4; two pairs per row (option "lin_pairs"): rows
inline long lin_count(int mode, bool pairs, int N, long Bp)
{
    if (mode == 4) return Bp;
    if (!pairs) return (long)(N + 1) * Bp;
    return mode == 3 ? lin_pair_retire_rows(N, Bp) : lin_pair_plain_rows(N, Bp);
}
// (MODE 4: a wave per group; else a 16-lane row per pair, item or row of pairs)
constexpr int lin_per_block(int mode) { return mode == 4 ? lin_block(mode) / LIN_WAVE : lin_block(mode) / LIN_GROUP_LANES; }
// words of DevPtrs::redo per instance: one bit per stage 0 .. N
constexpr int redo_words(int N) { return (N + 32) / 32; }

struct LinLaunch { // usv_linearize<MODE><<<blocks, block>>>(ptrs, count)
    int mode;
    long blocks;
    int block;
    long count;
};
inline LinLaunch lin_launch(int mode, bool pairs, int N, long Bp)
{
    const long n = lin_count(mode, pairs, N, Bp), per_block = lin_per_block(mode);
    return LinLaunch{mode, (n + per_block - 1) / per_block, lin_block(mode), n};
}

// A group -> instance map, by the buffer that holds it
enum LinMap {
    MAP_NONE = 0, // the identity (no buffer)
    MAP_A,        // usvmpc_handle::d_perm
    MAP_B         // ... d_perm2 (exists once the pipeline has run)
};

// The linearisation made a tick ahead: is there one, for which solve, under which map, and is it still good?  Every writer of that answer is
// a method here; the handle holds one LinSched and assigns none of its fields.
struct LinSched {
    long tick;        // number of the solve plan_lin planned last
    long made_for;    // solve number the outstanding / finished speculative linearisation was made for (-1: none)
    bool valid;       // ... and nothing it read has been changed by the caller since
    bool outstanding; // the second stream may still be writing the lineariser's planes
    int quiet;        // RTI solves in a row whose ahead-of-time linearisation (had there been one) no caller write invalidated (SPEC_QUIET_MIN)
    LinMap map;       // the group -> instance map it used (= the map the solve made_for must use)
    bool fine;        // ... made by usv_linearize MODE 3 (its fix-up is MODE 4) instead of MODE 1 (MODE 2): launched_ahead
    long hits, misses; // ahead-of-time linearisations used / discarded (usvmpc_pipeline_stats)

    void reset()
    {
        tick = 0; made_for = -1; valid = false; outstanding = false; quiet = 0; map = MAP_NONE; fine = false;
        hits = 0; misses = 0;
    }
    // The caller replaced x / u / yref / yref_e: a lineariser that ran ahead may have read what is being replaced - the next solve linearises
    // again.  (A handle that keeps a host mirror never pipelines - plan_lin - and a mirror that was given up does not come back: `valid` is
    // never set where a write goes to the mirror, and clearing it there as well changes nothing.)
    void caller_wrote() { valid = false; quiet = 0; }
    // Something the pass made ahead read or wrote is about to change (an option, a map, a caller's device pointer): forget what it made.
    // True: it may still be running - the executor synchronises the second stream, once.
    bool cancel()
    {
        caller_wrote();
        const bool wait = outstanding;
        outstanding = false;
        return wait;
    }
    // The executor has waited for both streams (usvmpc_sync: the lineariser that runs a tick ahead is part of the work enqueued so far)
    void synced() { outstanding = false; }
    // The next tick's lineariser went out on the second stream, behind the QP launch of the solve planned last and under next_map.  Returns
    // its MODE - known only now, because plan_qp decides the hand-over inside launch_qp.
    // Which form: in the retire order, by one-wave workgroups (MODE 3, fix-up MODE 4), when this QP launch hands nothing over.  A launch
    // that does (batches up to three times the resident rows) needs the slots its leaving waves free for its follow-up workgroups, a
    // large share of its instances is still running when the lineariser arrives, and the fix-up has a large share to redo: measured
    // at 16 384 instances the fine form cost 0.6 ms of QP launch and 0.35 ms of fix-up per 21 ms tick; at 65 536 it saves 1.4 of 71.5 ms.
    int launched_ahead(bool hands_over, LinMap next_map)
    {
        fine = !hands_over;
        made_for = tick + 1;
        valid = true;
        outstanding = true;
        map = next_map;
        return fine ? 3 : 1;
    }
};

struct LinIn {
    int phase;                // 0: an RTI solve; 1, 2: the launches of a full SQP
    long nsolves;             // solves launched so far = this solve's number
    int B, Bp, N;
    // options
    bool pipeline, dynamic_rows, sort_enabled, sort_two;
    int lin_force;            // option "lin_force_modes" (tests)
    bool pairs;               // option "lin_pairs"
    bool cond;                // option "qp_cond_N" > 0: RTI solves go through the partially condensed QP
    // the handle
    bool mirror;              // it keeps a host mirror
    bool extern_access;       // a device pointer was handed out
    LinMap cur_map;           // the map the previous solve ran under (DevPtrs::perm)
};

struct LinPlan {
    bool pipe;                // the pipeline applies to this solve: the second stream and its buffers are wanted
    bool wait_ahead;          // first of all the stream waits for the pass made ahead (it may still be writing the lineariser's planes)
    bool use_ahead;           // the pass made ahead for this solve stands: only its fix-up runs
    // the map this solve runs under
    enum { KEEP, AHEAD, SORT } map_from; // as it is | the one the pass made ahead used | sorted now, into buffer A
    LinMap map;               // ... which is then this one
    bool map_changed;         // usvmpc_handle::map_changed is to be set
    bool spec_next;           // the next tick's lineariser runs ahead, beside this solve's QP launch (DevPtrs::epoch on)
    bool redo;                // DevPtrs::redo on ...
    bool clear_redo;          // ... and cleared behind this solve's lineariser
    // this solve's lineariser, on the main stream
    int nlaunch;
    LinLaunch launch[2];
    bool forced;              // option "lin_force_modes": the launches run on private epoch / redo buffers, epoch filled with force_epoch
    int force_epoch;
    int pair_launches;        // how many of them are paired kernels (usvmpc_lin_pair_launches)
    bool sort_next;           // the next tick's map is sorted now ...
    LinMap next_map;          // ... into this buffer (MAP_NONE: the pass made ahead runs under the identity)
    bool copy_iter_prev;      // the counts of the solve before this one are kept as the second half of the next sort key
};

// What a solve does with the lineariser, ahead of its QP launch.  Moves `s` on: the pass made ahead is consumed, hit or miss counted.
inline LinPlan plan_lin(const LinIn &in, LinSched &s)
{
    LinPlan p = {};
    // Pipelined: RTI solves of large handles without a host mirror whose arrays no caller writes behind the library's back
    p.pipe = in.phase == 0 && in.pipeline && !in.mirror && !in.extern_access && in.dynamic_rows && in.B >= PIPELINE_MIN_BATCH && !in.cond;
    // whatever this solve does with the lineariser's planes comes after a speculative linearisation that may still be writing them
    p.wait_ahead = s.outstanding;
    s.outstanding = false;
    const bool had = p.pipe && s.made_for == in.nsolves;
    p.use_ahead = had && s.valid;
    if (had) (p.use_ahead ? s.hits : s.misses)++;
    s.valid = false;
    s.tick = in.nsolves;
    p.map_from = LinPlan::KEEP;
    p.map = in.cur_map;
    if (p.use_ahead) {
        // the map this tick was linearised under (made one tick ago from the counts of the solve before); the workspace's multipliers
        // count as written under another map even when that map is the identity again (sorting off)
        p.map_from = LinPlan::AHEAD;
        p.map = s.map;
        p.map_changed = true;
    } else if (in.sort_enabled && in.nsolves > 0 && in.phase != 2) {
        // (the later iterations of a full SQP read the multipliers the previous launch left in the group-indexed workspace: the
        // group -> instance map must not change inside one SQP call; a phase-1 launch re-sorts BEFORE its QP writes the multipliers:
        // map and workspace stay consistent)
        p.map_from = LinPlan::SORT;
        p.map = MAP_A;
        p.map_changed = in.phase == 0;
    }
    if (p.pipe) s.quiet++; // (reset by every caller write that would invalidate a linearisation made ahead of time)
    // The next tick's lineariser runs ahead: behind this solve's QP launch, on the second stream.  That stream has the lowest priority: when
    // its lineariser and the main stream's QP launch become eligible together, the QP launch's workgroups are placed first and the lineariser
    // gets the compute units that launch vacates; groups it reaches before their instance is final are marked and redone by the fix-up pass -
    // measured on the bench workload: 0.35 of 7.4 ms, ~5 % of the groups.
    p.spec_next = p.pipe && s.quiet >= SPEC_QUIET_MIN;
    p.redo = p.pipe;
    p.clear_redo = p.pipe;
    // (MODE 2 / 4: only what the speculative pass had to skip)
    const int mode = p.use_ahead ? (s.fine ? 4 : 2) : 0;
    // Option "lin_force_modes" (tests): a solve that would run the whole-batch lineariser runs the pipeline's kernels MODE 3 + MODE 4 in its
    // place - 1: with every instance final (epoch = this tick), 2: with none (-1)
    p.forced = in.lin_force != 0 && mode == 0 && in.phase == 0;
    if (p.forced) {
        p.force_epoch = in.lin_force == 1 ? (int)in.nsolves : -1;
        p.launch[0] = lin_launch(3, in.pairs, in.N, in.Bp);
        p.launch[1] = lin_launch(4, in.pairs, in.N, in.Bp);
        p.nlaunch = 2;
    } else {
        p.launch[0] = lin_launch(mode, in.pairs, in.N, in.Bp);
        p.nlaunch = 1;
    }
    p.pair_launches = in.pairs ? p.nlaunch : 0;
    // the NEXT tick's map, from the counts this launch is about to overwrite, into the buffer this tick does not use
    p.sort_next = p.spec_next && in.sort_enabled;
    p.next_map = !p.sort_next ? MAP_NONE : (p.map == MAP_A ? MAP_B : MAP_A);
    // (copied after every sort of THIS solve has read the pair (qp_iter, d_iter_prev), the pipelined map's included, and before the QP
    // launch overwrites qp_iter)
    p.copy_iter_prev = in.sort_enabled && in.sort_two && in.phase == 0;
    return p;
}

} // namespace usv
