// log_plan.hpp — the closed-loop log (include/usvmpc.h: usvmpc_log_*): which hand-over makes a record, where a record lies and what a read
// copies, as host-only code.  No HIP header and no pointer: usvmpc.hip's log_handover asks LogPlan::on_handover what this hand-over does and
// launches usv_log_record accordingly, usvmpc_log_read carries out the copy read_desc describes; tests/log_plan_harness.cpp drives the same
// code from a command line (tests/test_log_plan.py).  The arithmetic of the kernel: closed_loop_log.hpp.
//
// A log is three channels of `capacity` records each, tick-major, plus two running sums per (instance, error channel):
//     x       [capacity][B][nsel]  doubles   the selected states of x0 at the hand-over (the reference's simX[i])
//     u       [capacity][B][nu]    doubles   u of stage 0 (simU[i])
//     status  [capacity][B]        int32     status | qp_iter << 8 of the last solve
//     sum_abs, sum_sq  [B][n_err]  doubles   sums of |e| and e e over the hand-overs from err_first on
// Hand-over i (counted from the start of the log) makes a record when i >= first, (i - first) % every == 0 and a slot is free; with the
// buffer full it counts as missed.  No ring: a log that is full stays as it is.
#pragma once

#include <cmath>
#include <cstring>

namespace usv {

constexpr int LOG_ERR_MAX = 4;   // error channels
constexpr int LOG_SEL_MAX = 16;  // states a record can hold: the selection travels as a list of 4-bit indices in 64 bits

// (the fields of usvmpc_log_desc)
struct LogDesc {
    int capacity, every, first;
    unsigned state_mask;
    int record_u, record_status;
    int n_err;
    int err_a[LOG_ERR_MAX], err_b[LOG_ERR_MAX];
    double err_c[LOG_ERR_MAX];
    int err_first;
};

inline int log_popcount(unsigned m)
{
    int n = 0;
    for (; m; m &= m - 1) n++;
    return n;
}

// bytes of the channels; a channel that is not recorded has none
struct LogLayout {
    int B, nsel, nu, n_err, capacity;
    long long x_bytes, u_bytes, status_bytes, sums_bytes; // (sums_bytes: sum_abs and sum_sq together, sum_sq behind sum_abs)
    long long total() const { return x_bytes + u_bytes + status_bytes + sums_bytes; }
};

// a * b * c * d in 64 bits; false: it does not fit
inline bool log_size(long long a, long long b, long long c, long long d, long long *out)
{
    long long r;
    if (__builtin_mul_overflow(a, b, &r) || __builtin_mul_overflow(r, c, &r) || __builtin_mul_overflow(r, d, &r)) return false;
    *out = r;
    return true;
}

// nullptr: the descriptor is good for a handle of these sizes and *lay is its layout; else why not
inline const char *check_log_desc(const LogDesc &d, int nx, int nu, int B, LogLayout *lay)
{
    if (nx < 1 || nx > LOG_SEL_MAX || nu < 0 || B < 1) return "log: a model of 1 .. 16 states and a batch of at least 1 are needed";
    if (d.capacity < 1) return "log: capacity must be at least 1";
    if (d.every < 1) return "log: every must be at least 1";
    if (d.first < 0) return "log: first must not be negative";
    if (nx < 32 && (d.state_mask >> nx) != 0u) return "log: state_mask names a state the model does not have";
    if (d.n_err < 0 || d.n_err > LOG_ERR_MAX) return "log: n_err must lie in 0 .. 4";
    for (int c = 0; c < d.n_err; c++) {
        if (d.err_a[c] < 0 || d.err_a[c] >= nx) return "log: err_a must name a state of the model";
        if (d.err_b[c] >= nx) return "log: err_b must name a state of the model or be negative";
        if (d.err_b[c] < 0 && !std::isfinite(d.err_c[c])) return "log: err_c must be finite";
    }
    const int nsel = log_popcount(d.state_mask);
    const bool rec_u = d.record_u != 0 && nu > 0, rec_s = d.record_status != 0;
    if (nsel == 0 && !rec_u && !rec_s && d.n_err == 0) return "log: the descriptor records nothing";
    LogLayout l = {};
    l.B = B; l.nsel = nsel; l.nu = rec_u ? nu : 0; l.n_err = d.n_err; l.capacity = d.capacity;
    const char *big = "log: the log's size overflows";
    if (!log_size(d.capacity, B, nsel, (long long)sizeof(double), &l.x_bytes)) return big;
    if (!log_size(d.capacity, B, l.nu, (long long)sizeof(double), &l.u_bytes)) return big;
    if (!log_size(d.capacity, B, rec_s ? 1 : 0, (long long)sizeof(int), &l.status_bytes)) return big;
    if (!log_size(2, B, d.n_err, (long long)sizeof(double), &l.sums_bytes)) return big;
    long long t;
    if (__builtin_add_overflow(l.x_bytes, l.u_bytes, &t) || __builtin_add_overflow(t, l.status_bytes, &t) ||
        __builtin_add_overflow(t, l.sums_bytes, &t))
        return big;
    if (lay) *lay = l;
    return nullptr;
}

enum LogChannel { LOG_X = 0, LOG_U, LOG_STATUS, LOG_CHANNELS };

// what a hand-over does
struct LogTick {
    int slot;    // record to write, or -1
    bool errors; // the sums take this hand-over in
    bool missed; // it was due for a record and the buffer is full
};

// one 2-D copy out of a channel: `rows` runs of `width` bytes, `pitch` bytes apart, the first at `offset`
struct LogCopy {
    LogChannel channel;
    int n;          // values per (record, instance)
    int elem;       // bytes of a value
    long long offset, pitch, width, rows;
    long long bytes() const { return width * rows; }
};

// The log of a handle: is there one, what does it hold so far.  Every writer of the counters is a method here; the handle holds one LogPlan
// and assigns none of its fields.
struct LogPlan {
    bool on = false;
    LogDesc d = {};
    LogLayout lay = {};
    int records = 0;            // records made
    long long handovers = 0;    // hand-overs since start
    long long missed = 0;       // hand-overs due for a record that found the buffer full
    long long err_count = 0;    // hand-overs the sums took in

    void start(const LogDesc &desc, const LogLayout &layout)
    {
        on = true; d = desc; lay = layout;
        records = 0; handovers = 0; missed = 0; err_count = 0;
    }
    void stop() { on = false; }

    LogTick on_handover()
    {
        LogTick t = {-1, false, false};
        if (!on) return t;
        const long long i = handovers++;
        const bool channels = lay.x_bytes || lay.u_bytes || lay.status_bytes;
        if (channels && i >= d.first && (i - d.first) % d.every == 0) {
            if (records < d.capacity) t.slot = records++;
            else { t.missed = true; missed++; }
        }
        if (d.n_err > 0 && i >= d.err_first) { t.errors = true; err_count++; }
        return t;
    }

    // the copy behind usvmpc_log_read (nullptr), or why there is none
    const char *read_desc(const char *channel, long long rec0, long long nrec, long long b0, long long nb, LogCopy *out) const
    {
        if (!on) return "log: no log is running (usvmpc_log_start)";
        LogCopy c = {};
        long long have;
        if (channel && !std::strcmp(channel, "x")) { c.channel = LOG_X; c.n = lay.nsel; c.elem = (int)sizeof(double); have = lay.x_bytes; }
        else if (channel && !std::strcmp(channel, "u")) { c.channel = LOG_U; c.n = lay.nu; c.elem = (int)sizeof(double); have = lay.u_bytes; }
        else if (channel && !std::strcmp(channel, "status")) { c.channel = LOG_STATUS; c.n = 1; c.elem = (int)sizeof(int); have = lay.status_bytes; }
        else return "log: the channels are \"x\", \"u\" and \"status\"";
        if (have == 0) return "log: this channel is not recorded";
        if (rec0 < 0 || nrec < 1 || rec0 > records || nrec > records - rec0) return "log: records outside those made so far";
        if (b0 < 0 || nb < 1 || b0 > lay.B || nb > lay.B - b0) return "log: instances outside the batch";
        const long long cell = (long long)c.n * c.elem; // (the whole channel fits in 64 bits: check_log_desc)
        c.pitch = lay.B * cell;
        c.offset = rec0 * c.pitch + b0 * cell;
        c.width = nb * cell;
        c.rows = nrec;
        *out = c;
        return nullptr;
    }
};

} // namespace usv
