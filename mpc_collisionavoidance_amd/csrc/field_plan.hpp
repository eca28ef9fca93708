// field_plan.hpp — the caller-visible fields (usvmpc_set / _get / _get_int / _get_device_ptr) as ONE table, the layout of the arena that holds
// the arrays a caller sets, and the bookkeeping of the pinned host mirror of that arena as a host-only state machine (HostMirror).  No HIP
// header and no pointer: everything here works in byte offsets into the arena.  usvmpc.hip's copy_field resolves a name here, validates once
// and carries out the copies HostMirror names; tests/field_plan_harness.cpp drives the same code from a command line.
#pragma once

#include <cstddef>
#include <cstring>
#include <vector>

namespace usv {

// ---- 1. the field table
// The first ARENA_FIELDS ids are the arena's slots, in the arena's order [x | u | status | x0 | yref | yref_e | p | lh]
enum FieldId {
    FLD_X = 0, FLD_U, FLD_STATUS, FLD_X0, FLD_YREF, FLD_YREF_E, FLD_P, FLD_LH, ARENA_FIELDS,
    FLD_PI = ARENA_FIELDS, FLD_SL, FLD_SU, FLD_RES, FLD_OBS_TMIN, FLD_NLP_RES, FLD_LAM, FLD_T, FLD_QP_ITER, FLD_QP_STATUS, FLD_SQP_ITER,
    FLD_OBS_POS, FLD_OBS_VEL, FLD_CLEARANCE, FLD_CLEARANCE_MIN, FLD_COST, FLD_COST_STAGE, FLD_COST_PARTS, FLD_COUNT
};
enum FieldLen { LEN_NX, LEN_NU, LEN_NY, LEN_NY_E, LEN_2K, LEN_K, LEN_NLAM, LEN_4, LEN_3, LEN_1 }; // per-stage length, over the handle's sizes
enum FieldStages { ST_N1, ST_N, ST_1 };                                                      // N + 1 | N | 1
enum : unsigned { // rights
    R_SET = 1,     // usvmpc_set
    R_GET = 2,     // usvmpc_get
    R_GET_INT = 4, // usvmpc_get_int
    R_DEV = 8      // usvmpc_get_device_ptr
};
enum : unsigned { // flags
    FF_WHOLE = 1,  // whole-only: one row per instance, whatever stage the caller names (normalised to stage < 0 ? -1 : 0)
    FF_LIN = 2,    // read by the lineariser: a caller write invalidates the pass made a tick ahead (LinSched::caller_wrote)
    FF_PF = 4,     // owned by the path-following front end: a caller write makes it rewrite its rows (usvmpc_handle::pf_stale)
    FF_EXPORT = 8, // a multiplier read-back: the export runs first, and the field exists only once its buffers do (FieldDims::exported)
    FF_TRACK = 16, // an obstacle-track field (usvmpc.hip: tracks_field)
    FF_COST = 32   // an objective value: evaluated by usv_cost_eval ahead of the copy, into buffers made on first use (usvmpc.hip: cost_enqueue)
};

struct FieldRow {
    const char *name;
    FieldId id;
    int slot;          // arena slot, -1: not in the arena
    bool is_int;       // element type: int instead of double
    FieldLen len;
    FieldStages stages;
    bool from_1;       // the caller's stage of slot 0 is 1 instead of 0
    unsigned rights, flags;
};

constexpr FieldRow FIELD_TABLE[FLD_COUNT] = {
    // name            id                 slot         int    length    stages from_1 rights                  flags
    {"x",             FLD_X,             FLD_X,       false, LEN_NX,   ST_N1, false, R_SET | R_GET | R_DEV,  FF_LIN},
    {"u",             FLD_U,             FLD_U,       false, LEN_NU,   ST_N,  false, R_SET | R_GET | R_DEV,  FF_LIN},
    {"status",        FLD_STATUS,        FLD_STATUS,  true,  LEN_1,    ST_1,  false, R_GET_INT | R_DEV,      0},
    {"x0",            FLD_X0,            FLD_X0,      false, LEN_NX,   ST_1,  false, R_SET | R_GET | R_DEV,  FF_WHOLE},
    {"yref",          FLD_YREF,          FLD_YREF,    false, LEN_NY,   ST_N,  false, R_SET | R_GET | R_DEV,  FF_LIN | FF_PF}, // (stage N: yref_e - resolve)
    {"yref_e",        FLD_YREF_E,        FLD_YREF_E,  false, LEN_NY_E, ST_1,  false, R_SET | R_GET | R_DEV,  FF_WHOLE | FF_LIN | FF_PF},
    {"p",             FLD_P,             FLD_P,       false, LEN_2K,   ST_N1, false, R_SET | R_GET | R_DEV,  0},
    {"lh",            FLD_LH,            FLD_LH,      false, LEN_K,    ST_N,  false, R_SET | R_GET | R_DEV,  0},
    {"pi",            FLD_PI,            -1,          false, LEN_NX,   ST_N,  true,  R_GET | R_DEV,          0},
    {"sl",            FLD_SL,            -1,          false, LEN_K,    ST_N,  false, R_GET | R_DEV,          0},
    {"su",            FLD_SU,            -1,          false, LEN_K,    ST_N,  false, R_GET | R_DEV,          0},
    {"res",           FLD_RES,           -1,          false, LEN_4,    ST_1,  false, R_GET | R_DEV,          FF_WHOLE},
    {"obs_tmin",      FLD_OBS_TMIN,      -1,          false, LEN_1,    ST_1,  false, R_GET | R_DEV,          FF_WHOLE},
    {"nlp_res",       FLD_NLP_RES,       -1,          false, LEN_4,    ST_1,  false, R_GET | R_DEV,          FF_WHOLE},
    {"lam",           FLD_LAM,           -1,          false, LEN_NLAM, ST_N1, false, R_GET,                  FF_EXPORT},
    {"t",             FLD_T,             -1,          false, LEN_NLAM, ST_N1, false, R_GET,                  FF_EXPORT},
    {"qp_iter",       FLD_QP_ITER,       -1,          true,  LEN_1,    ST_1,  false, R_GET_INT | R_DEV,      0},
    {"qp_status",     FLD_QP_STATUS,     -1,          true,  LEN_1,    ST_1,  false, R_GET_INT | R_DEV,      0},
    {"sqp_iter",      FLD_SQP_ITER,      -1,          true,  LEN_1,    ST_1,  false, R_GET_INT | R_DEV,      0},
    // (the stage of a track field is ignored: tracks_field)
    {"obs_pos",       FLD_OBS_POS,       -1,          false, LEN_2K,   ST_1,  false, R_SET | R_GET | R_DEV,  FF_TRACK},
    {"obs_vel",       FLD_OBS_VEL,       -1,          false, LEN_2K,   ST_1,  false, R_SET | R_GET | R_DEV,  FF_TRACK},
    {"clearance",     FLD_CLEARANCE,     -1,          false, LEN_1,    ST_1,  false, R_GET,                  FF_TRACK},
    {"clearance_min", FLD_CLEARANCE_MIN, -1,          false, LEN_1,    ST_1,  false, R_GET,                  FF_TRACK},
    // (the objective value of the iterate the handle holds: cost_eval.hpp)
    {"cost",          FLD_COST,          -1,          false, LEN_1,    ST_1,  false, R_GET | R_DEV,          FF_WHOLE | FF_COST},
    {"cost_stage",    FLD_COST_STAGE,    -1,          false, LEN_1,    ST_N1, false, R_GET | R_DEV,          FF_COST},
    {"cost_parts",    FLD_COST_PARTS,    -1,          false, LEN_3,    ST_1,  false, R_GET | R_DEV,          FF_WHOLE | FF_COST},
};

constexpr bool field_table_ordered()
{
    for (int i = 0; i < FLD_COUNT; i++)
        if (FIELD_TABLE[i].id != i || FIELD_TABLE[i].slot != (i < ARENA_FIELDS ? i : -1)) return false;
    return true;
}
static_assert(field_table_ordered(), "FIELD_TABLE[id] is the row of id, and the arena's slots come first");

// the row of a name; nullptr: no such field (a null name included)
inline const FieldRow *find_field(const char *name)
{
    if (name)
        for (const FieldRow &r : FIELD_TABLE)
            if (std::strcmp(r.name, name) == 0) return &r;
    return nullptr;
}

struct FieldDims { // the handle's sizes
    int N, nx, nu, ny, ny_e, K;
    int nlam;      // rows of "lam" / "t" per stage ...
    bool exported; // ... which exist only once their buffers do (DevPtrs::lam_out / t_out)
};
inline int field_len(const FieldRow &r, const FieldDims &d)
{
    switch (r.len) {
    case LEN_NX: return d.nx;
    case LEN_NU: return d.nu;
    case LEN_NY: return d.ny;
    case LEN_NY_E: return d.ny_e;
    case LEN_2K: return 2 * d.K;
    case LEN_K: return d.K;
    case LEN_NLAM: return d.nlam;
    case LEN_4: return 4;
    case LEN_3: return 3;
    case LEN_1: break;
    }
    return 1;
}
inline int field_stages(const FieldRow &r, const FieldDims &d) { return r.stages == ST_N1 ? d.N + 1 : r.stages == ST_N ? d.N : 1; }

constexpr int FIELD_E_UNKNOWN = -2; // (USVMPC_E_FIELD: usvmpc.hip asserts it)

struct Field { // a row with its lengths filled in, for one usvmpc_set / usvmpc_get
    const FieldRow *row;
    int n;         // per-stage length
    int stages;    // number of stages in the array
    int stage_off; // caller stage that maps to slot 0
    int stage;     // the caller's stage, normalised for a whole-only field
};

// usvmpc_set (set) / usvmpc_get of `row` at `stage`: 0 and the field, or FIELD_E_UNKNOWN - no such name, no such right (an output is not
// settable, an integer field is not read as doubles), a multiplier read-back whose buffers do not exist.
// "yref" at stage N is "yref_e" (acados' cost_set(N, "yref")), addressed as that field's only stage.
inline int resolve(const FieldRow *row, int stage, const FieldDims &d, bool set, Field &o)
{
    if (!row || !(row->rights & (set ? R_SET : R_GET)) || ((row->flags & FF_EXPORT) && !d.exported)) return FIELD_E_UNKNOWN;
    if (row->flags & FF_WHOLE) stage = stage < 0 ? -1 : 0;
    int off = row->from_1 ? 1 : 0;
    if (row->id == FLD_YREF && stage == d.N) { row = &FIELD_TABLE[FLD_YREF_E]; off = d.N; }
    o = Field{row, field_len(*row, d), field_stages(*row, d), off, stage};
    return 0;
}
inline int resolve(const char *name, int stage, const FieldDims &d, bool set, Field &o) { return resolve(find_field(name), stage, d, set, o); }

// the stage of a resolved field: 0 fine; 1: "stage <s> out of range for field '<name>'"; 2: "stage out of range" (a one-stage array asked
// for another stage than its own)
inline int stage_check(const Field &f)
{
    const int slot = f.stage - f.stage_off;
    if (f.stage < 0) return 0;
    if (f.stages == 1) return slot != 0 ? 2 : 0;
    return slot < 0 || slot >= f.stages ? 1 : 0;
}

// A copy: `rows` pieces of `width` bytes, `pitch` bytes apart, the first `off` bytes into the arena (HostMirror) or into the field
// (field_span); rows == 1 is a 1-D copy
struct CopyDesc {
    size_t off, pitch, width, rows;
};

// what a set / get of a (checked) field touches inside its [B][stages][n] array: the whole array as one piece, or one stage of every instance
inline CopyDesc field_span(const Field &f, size_t B, size_t elem = sizeof(double))
{
    const size_t row = (size_t)f.n * elem, pitch = (size_t)f.stages * row;
    if (f.stage < 0 || f.stages == 1) return CopyDesc{0, B * pitch, B * pitch, 1};
    return CopyDesc{(size_t)(f.stage - f.stage_off) * row, pitch, row, B};
}

// ---- 2. the arena: the arrays a caller sets and the results of a solve in ONE device allocation, 256-byte aligned pieces in slot order
constexpr size_t MIRROR_MAX = 1u << 20; // arenas up to 1 MiB are mirrored on the host

struct ArenaLayout {
    size_t B;
    size_t off[ARENA_FIELDS + 1]; // (the last one: the arena's size)
    size_t len[ARENA_FIELDS];
    size_t stages[ARENA_FIELDS];
    size_t bytes() const { return off[ARENA_FIELDS]; }
};
inline ArenaLayout arena_layout(const FieldDims &d, size_t B)
{
    ArenaLayout a = {};
    a.B = B;
    size_t off = 0;
    for (int s = 0; s < ARENA_FIELDS; s++) {
        const FieldRow &r = FIELD_TABLE[s];
        a.stages[s] = (size_t)field_stages(r, d);
        a.len[s] = B * a.stages[s] * (size_t)field_len(r, d) * (r.is_int ? sizeof(int) : sizeof(double));
        a.off[s] = off;
        off += (a.len[s] + 255) / 256 * 256;
    }
    a.off[ARENA_FIELDS] = off;
    return a;
}

// ---- 3. the host mirror
// Small handles (the single-instance drop-in faces: AcadosOcpSolver, the acados C shim) keep a pinned host MIRROR of the arena: usvmpc_set
// then writes the mirror and marks the field dirty - no HIP call, no synchronisation - and the next launch uploads what is dirty (the
// reference protocol's 3N+4 setters per tick become ONE asynchronous copy: the dirty fields are adjacent); after a solve [x | u | status]
// comes back in ONE copy and usvmpc_get "x" / "u" is served from it.
// What is dirty, what is in flight and whom the mirror may answer is this struct; every writer of it is a method here (the handle holds one
// HostMirror and assigns none of its fields), and what a method wants copied it returns as CopyDescs for the executor in usvmpc.hip.
//
// Two properties of this bookkeeping are kept as they were found - both may deserve a change of behaviour, neither is made here
// (tests/test_field_plan.py pins them):
//   (a) With B == 1 a field has ONE dirty range: two sets of non-adjacent stages upload everything in between from the mirror as well -
//       stale where a device-side writer has written those stages behind the mirror since.
//   (b) The rule "a handed-out device pointer makes the upload immediate" exists for strided stages only (B > 1): with B == 1, or for a
//       whole-field set, the set stays deferred until the next launch even while a caller holds a device pointer.
struct HostMirror {
    ArenaLayout lay;
    bool on;           // the handle keeps a mirror (arena at most MIRROR_MAX; given up by option "host_mirror" 0 and never taken up again)
    size_t dirty_lo[ARENA_FIELDS], dirty_hi[ARENA_FIELDS]; // byte range inside each field that the mirror holds newer than the device (lo >= hi: none)
    // one stage of several instances set at a time (the reference protocol on a small multi-instance handle): the rows of that stage are not
    // contiguous, so they are remembered per (field, stage) and go up at the next launch as 2-D copies of runs of consecutive stages
    std::vector<char> dirty_stage[ARENA_FIELDS]; // (sized once, in reset: no allocation on the set path)
    bool any_stage[ARENA_FIELDS];
    bool inflight;     // a copy between mirror and arena may still be running on the stream
    bool out_valid;    // the mirror's [x | u | status] is what the device holds (or newer)
    bool extern_access; // a device pointer was handed out: the device arrays may change behind the mirror

    void reset(const ArenaLayout &l, bool keep)
    {
        lay = l;
        on = keep;
        for (int s = 0; s < ARENA_FIELDS; s++) {
            dirty_lo[s] = 1; dirty_hi[s] = 0;
            dirty_stage[s].assign(lay.stages[s], 0);
            any_stage[s] = false;
        }
        inflight = false; out_valid = false; extern_access = false;
    }

    // ---- whether a call is served by the mirror (else: by a copy from / to the device, synchronised)
    // every set of an arena field
    bool set_served(int slot) const { return on && slot >= 0; }
    // a get of x / u, while what came back with the last solve is still what the device holds - not once a device pointer is out; and status
    // for usvmpc_solve, which reads it right behind its own synchronise, when what came back is that solve's whatever the caller holds.
    // (x0, yref .. lh are never served: the device may have written them - usvmpc_advance, the guidance front ends)
    bool get_served(int slot) const { return on && out_valid && (slot == FLD_STATUS || ((slot == FLD_X || slot == FLD_U) && !extern_access)); }
    // ... and the host first waits for the stream (then: synced), because a copy may still be reading or writing the mirror
    bool must_wait() const { return inflight; }

    // ---- what a set leaves behind: `span` of field `slot` (field_span) has been written into the mirror.  True: `now` goes up at once.
    bool wrote(int slot, const CopyDesc &span, CopyDesc &now)
    {
        if (span.rows > 1) {
            // one stage of several instances: the rows are not contiguous, and a dirty RANGE over them would later upload the mirror's
            // copy of everything in between - stale where a device-side writer (the guidance kernels, a caller holding a device pointer)
            // has written behind the mirror.  The stage is remembered; its rows go up with the next launch (next_upload), as one 2-D copy
            // per run of consecutive dirty stages - no HIP call here (the immediate copy made the NEXT set synchronise)
            // A caller that holds device pointers (usvmpc_get_device_ptr: extern_access) orders its own kernels against this set by the
            // stream: for it the rows go up NOW, as before (a deferred upload would land on top of what the caller's kernel
            // wrote to the same stage after the set, and a caller kernel reading the field before the solve would see the old rows).
            if (extern_access) {
                now = CopyDesc{lay.off[slot] + span.off, span.pitch, span.width, span.rows};
                inflight = true;
                return true;
            }
            dirty_stage[slot][span.off / span.width] = 1;
            any_stage[slot] = true;
            return false;
        }
        // the whole field, or one stage of a single instance: the field's ONE range widens - properties (a) and (b) above
        const size_t lo = span.off, hi = span.off + span.width;
        if (dirty_lo[slot] >= dirty_hi[slot]) { dirty_lo[slot] = lo; dirty_hi[slot] = hi; }
        else {
            if (lo < dirty_lo[slot]) dirty_lo[slot] = lo;
            if (hi > dirty_hi[slot]) dirty_hi[slot] = hi;
        }
        return false;
    }

    // ---- flush: what the mirror holds newer than the device, one copy per call until false; everything is clean then.  First one 2-D copy
    // per run of consecutive dirty stages (a whole-field range that is dirty as well goes up after them and covers these rows: same bytes,
    // the order does not matter), then the dirty ranges - consecutive dirty fields as ONE copy
    bool next_upload(CopyDesc &c)
    {
        if (!on) return false;
        for (int s = 0; s < ARENA_FIELDS; s++) {
            if (!any_stage[s]) continue;
            std::vector<char> &ds = dirty_stage[s];
            const size_t stages = ds.size(), pitch = lay.len[s] / lay.B, row = pitch / stages;
            size_t a = 0;
            while (a < stages && !ds[a]) a++;
            if (a == stages) { any_stage[s] = false; continue; }
            size_t b = a;
            while (b + 1 < stages && ds[b + 1]) b++;
            for (size_t i = a; i <= b; i++) ds[i] = 0;
            c = CopyDesc{lay.off[s] + a * row, pitch, (b - a + 1) * row, lay.B};
            inflight = true;
            return true;
        }
        for (int f = 0; f < ARENA_FIELDS; f++) {
            if (dirty_lo[f] >= dirty_hi[f]) continue;
            const size_t lo = lay.off[f] + dirty_lo[f];
            size_t hi = lay.off[f] + dirty_hi[f];
            // extend over the following fields while this one is dirty to its end and the next from its start
            int g = f;
            while (g + 1 < ARENA_FIELDS && dirty_hi[g] == lay.len[g] && dirty_lo[g + 1] == 0 && dirty_hi[g + 1] > 0) {
                g++;
                hi = lay.off[g] + dirty_hi[g];
            }
            for (int i = f; i <= g; i++) { dirty_lo[i] = 1; dirty_hi[i] = 0; }
            c = CopyDesc{lo, hi - lo, hi - lo, 1};
            inflight = true;
            return true;
        }
        return false;
    }

    // ---- the read-back after a solve: [x | u | status] of this solve come back as one copy (false: no mirror)
    bool read_back(CopyDesc &c)
    {
        if (!on) return false;
        c = CopyDesc{0, lay.off[FLD_X0], lay.off[FLD_X0], 1};
        inflight = true;
        out_valid = true;
        return true;
    }

    // the executor has waited for the stream: no copy is running
    void synced() { inflight = false; }
    // a device pointer to an arena field goes out (the executor has flushed): the mirror no longer vouches for the device's x / u
    void handed_out() { extern_access = true; }
    // the mirror is given up (the executor has flushed and waited)
    void dropped() { on = false; inflight = false; out_valid = false; }
};

} // namespace usv
