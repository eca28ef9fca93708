// cascade_log_plan.hpp — the log of the two-layer control stack (include/usvmpc.h: usvmpc_cascade_log_*): which low-level tick makes a
// record, where a record lies, what a read copies and how the status word is packed, as host-only code.  No HIP header and no pointer:
// usvmpc.hip's usvmpc_cascade_step asks CasLogPlan::on_tick what this tick does and launches usv_cascade_record accordingly,
// usvmpc_cascade_log_read carries out the copy read_desc describes; tests/cascade_log_plan_harness.cpp drives the same code from a command
// line (tests/test_cascade_log_plan.py).  The schedule and its counters are LogPlan's (log_plan.hpp), fed a descriptor without error channels.
//
// A log is five channels of `capacity` records each, tick-major:
//     state   [capacity][B][nsel]  doubles   the selected entries of the vessel state (nedx, nedy, psi, u, v, r) as the tick's low-level solve
//                                            saw it, before the plant period (the reference's simX[i])
//     thrust  [capacity][B][2]     doubles   the thrusts the tick publishes (zero while u_des = 0)
//     ref     [capacity][B][2]     doubles   the (heading, speed) the low level tracks at the tick
//     err     [capacity][B][2]     float32   (e_u, e_psi) of the tick
//     status  [capacity][B]        int32     cas_log_status_word of the two layers' last solves
// Tick i (counted from the start of the log) makes a record when i >= first, (i - first) % every == 0 and a slot is free; with the buffer
// full it counts as missed.  No ring: a log that is full stays as it is.
#pragma once

#include <cstring>

#include "log_plan.hpp"

#ifndef USV_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define USV_HD __host__ __device__ inline
#else
#define USV_HD inline
#endif
#endif

namespace usv {

constexpr int CAS_LOG_NS = 6;  // the vessel's states a record can select from

// (the fields of usvmpc_cascade_log_desc)
struct CasLogDesc {
    int capacity, every, first;
    unsigned state_mask;
    int record_thrust, record_ref, record_err, record_status;
};

// The status word: low-level status in bits 0-7 and qp_iter in bits 8-15, guidance status in bits 16-23 and qp_iter in bits 24-30.  Bit 31
// stays clear: the word is never negative.
USV_HD int cas_log_status_word(int ll_status, int ll_qp_iter, int g_status, int g_qp_iter)
{
    return (int)(((unsigned)ll_status & 0xffu) | (((unsigned)ll_qp_iter & 0xffu) << 8) | (((unsigned)g_status & 0xffu) << 16) |
                 (((unsigned)g_qp_iter & 0x7fu) << 24));
}

// bytes of the channels; a channel that is not recorded has none
struct CasLogLayout {
    int B, nsel, capacity;
    long long state_bytes, thrust_bytes, ref_bytes, err_bytes, status_bytes;
    long long total() const { return state_bytes + thrust_bytes + ref_bytes + err_bytes + status_bytes; }
};

// nullptr: the descriptor is good for a cascade of B instances and *lay is its layout; else why not
inline const char *check_cas_log_desc(const CasLogDesc &d, int B, CasLogLayout *lay)
{
    if (B < 1) return "log: a batch of at least 1 is needed";
    if (d.capacity < 1) return "log: capacity must be at least 1";
    if (d.every < 1) return "log: every must be at least 1";
    if (d.first < 0) return "log: first must not be negative";
    if ((d.state_mask >> CAS_LOG_NS) != 0u) return "log: state_mask names a state the vessel does not have";
    const int nsel = log_popcount(d.state_mask);
    const bool thr = d.record_thrust != 0, ref = d.record_ref != 0, err = d.record_err != 0, st = d.record_status != 0;
    if (nsel == 0 && !thr && !ref && !err && !st) return "log: the descriptor records nothing";
    CasLogLayout l = {};
    l.B = B; l.nsel = nsel; l.capacity = d.capacity;
    const char *big = "log: the log's size overflows";
    if (!log_size(d.capacity, B, nsel, (long long)sizeof(double), &l.state_bytes)) return big;
    if (!log_size(d.capacity, B, thr ? 2 : 0, (long long)sizeof(double), &l.thrust_bytes)) return big;
    if (!log_size(d.capacity, B, ref ? 2 : 0, (long long)sizeof(double), &l.ref_bytes)) return big;
    if (!log_size(d.capacity, B, err ? 2 : 0, (long long)sizeof(float), &l.err_bytes)) return big;
    if (!log_size(d.capacity, B, st ? 1 : 0, (long long)sizeof(int), &l.status_bytes)) return big;
    long long t;
    if (__builtin_add_overflow(l.state_bytes, l.thrust_bytes, &t) || __builtin_add_overflow(t, l.ref_bytes, &t) ||
        __builtin_add_overflow(t, l.err_bytes, &t) || __builtin_add_overflow(t, l.status_bytes, &t))
        return big;
    if (lay) *lay = l;
    return nullptr;
}

enum CasLogChannel { CAS_LOG_STATE = 0, CAS_LOG_THRUST, CAS_LOG_REF, CAS_LOG_ERR, CAS_LOG_STATUS, CAS_LOG_CHANNELS };

// one 2-D copy out of a channel: `rows` runs of `width` bytes, `pitch` bytes apart, the first at `offset`
struct CasLogCopy {
    CasLogChannel channel;
    int n;          // values per (record, instance)
    int elem;       // bytes of a value
    long long offset, pitch, width, rows;
    long long bytes() const { return width * rows; }
};

// The log of a cascade: is there one, what does it hold so far.  The schedule and the counters are a LogPlan's: every writer of them is a
// method of it, called from the methods here; the cascade holds one CasLogPlan and assigns none of its fields.
struct CasLogPlan {
    LogPlan sched;          // on, records, handovers (here: ticks), missed
    CasLogDesc d = {};
    CasLogLayout lay = {};

    bool on() const { return sched.on; }
    int records() const { return sched.records; }
    long long ticks() const { return sched.handovers; }
    long long missed() const { return sched.missed; }

    void start(const CasLogDesc &desc, const CasLogLayout &layout)
    {
        d = desc; lay = layout;
        // LogPlan's schedule of a descriptor without error channels; its layout only says that there is a channel to record (check_cas_log_desc
        // refuses a descriptor that records nothing, so total() > 0)
        LogDesc ld = {};
        ld.capacity = desc.capacity; ld.every = desc.every; ld.first = desc.first;
        LogLayout ll = {};
        ll.B = layout.B; ll.capacity = layout.capacity;
        ll.x_bytes = layout.total();
        sched.start(ld, ll);
    }
    void stop() { sched.stop(); }

    // what this low-level tick does: slot >= 0: record there; missed: it was due and the buffer is full
    LogTick on_tick() { return sched.on_handover(); }

    // the copy behind usvmpc_cascade_log_read (nullptr), or why there is none
    const char *read_desc(const char *channel, long long rec0, long long nrec, long long b0, long long nb, CasLogCopy *out) const
    {
        if (!on()) return "log: no log is running (usvmpc_cascade_log_start)";
        CasLogCopy c = {};
        long long have;
        const auto is = [&](const char *name) { return channel && !std::strcmp(channel, name); };
        if (is("state")) { c.channel = CAS_LOG_STATE; c.n = lay.nsel; c.elem = (int)sizeof(double); have = lay.state_bytes; }
        else if (is("thrust")) { c.channel = CAS_LOG_THRUST; c.n = 2; c.elem = (int)sizeof(double); have = lay.thrust_bytes; }
        else if (is("ref")) { c.channel = CAS_LOG_REF; c.n = 2; c.elem = (int)sizeof(double); have = lay.ref_bytes; }
        else if (is("err")) { c.channel = CAS_LOG_ERR; c.n = 2; c.elem = (int)sizeof(float); have = lay.err_bytes; }
        else if (is("status")) { c.channel = CAS_LOG_STATUS; c.n = 1; c.elem = (int)sizeof(int); have = lay.status_bytes; }
        else return "log: the channels are \"state\", \"thrust\", \"ref\", \"err\" and \"status\"";
        if (have == 0) return "log: this channel is not recorded";
        const long long made = records();
        if (rec0 < 0 || nrec < 1 || rec0 > made || nrec > made - rec0) return "log: records outside those made so far";
        if (b0 < 0 || nb < 1 || b0 > lay.B || nb > lay.B - b0) return "log: instances outside the batch";
        const long long cell = (long long)c.n * c.elem; // (the whole channel fits in 64 bits: check_cas_log_desc)
        c.pitch = lay.B * cell;
        c.offset = rec0 * c.pitch + b0 * cell;
        c.width = nb * cell;
        c.rows = nrec;
        *out = c;
        return nullptr;
    }
};

} // namespace usv
