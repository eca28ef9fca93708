// option_plan.hpp — the run-time options (usvmpc_set_option) as ONE table: every name with how its value is checked and normalised, where
// it is stored and what a change of it invalidates; the state they make up (Options, defaults included); and the pure function that turns
// (name, value, the handle's sizes) into a row, a normalised value or a refusal (parse_option).  No HIP header and no handle: usvmpc.hip's
// usvmpc_set_option looks the name up here, stores and carries out the row's effects (apply_option) and keeps the few hooks that need HIP
// or other handle state; tests/option_plan_harness.cpp drives the same code from a command line.
// Adding an option: a member of Options (or of DevSpec), a row here, its entry in include/usvmpc.h and its line in INTEGRATION.md
// (tests/test_option_plan.py looks for both).
#pragma once

#include "../../include/usvmpc.h" // (the return codes and USVMPC_HPIPM_*: plain C)

#include <cmath>
#include <cstddef>
#include <limits>
#include <string>

namespace usv {

// ---- 1. the options' state: one per handle (usvmpc_handle::opt).  The table below names every writer but two, which switch an option off
// on the handle's own authority: usvmpc_set_stream (pipeline, handover_co: nothing of the handle runs beside a caller's stream) and
// co_prepare (handover_co, when the co-resident kernel's stream cannot be made).  Options kept in DevSpec, where the kernels read them, are
// not here: "static_obstacles", "pack_box_rows", "cond_pred_corr", "cpc_factor", "hpipm_mode" (usvmpc.hip: store_option).
struct Options {
    bool pipeline = true;         // the lineariser of tick t + 1 runs on a second stream beside the QP launch of tick t (lin_plan.hpp); used for RTI solves of handles without a host mirror
    bool sort_enabled = true;     // instances are grouped by the IPM iteration count of their previous solve, hardest first
    bool sort_two = false;        // sort key: the larger of the last two iteration counts instead of the last one
    long max_waves = 0;           // cap on the persistent waves of the QP kernel (0: as many as the device holds)
    // (tests) a solve that would run the whole-batch lineariser runs the pipeline's kernels MODE 3 + MODE 4 in its place, on the main
    // stream - 1: the speculative form with every instance final, then the fix-up (which finds nothing); 2: with no instance final (it
    // marks everything), then the fix-up (which does everything).  Work order as in the pipeline, with the identity as the "running" map.
    int lin_force = 0;
    // the lineariser's kernels that serve two (group, stage) pairs per 16-lane row (usv_linearize PAIR; same bits) - the default for a
    // model that declares the columns to integrate (PairCols, params.hpp: defaults); 0: one pair per row
    int lin_pairs = 0;
    bool aux_lds = true;          // the aux plane of an RTI solve in the waves' LDS when the horizon fits
    int lds_mode = -1;            // workspace of the QP kernel in LDS: -1 when the batch is small enough, 0 never, 1 whenever it fits
    int wide_mode = -1;           // the latency mapping (one instance per wave, QpIpm WIDE): -1 for small batches, 0 never, 1 whenever it applies
    int wide_waves = -1;          // waves per instance of the latency mapping: -1 four for soft-row OCPs and two obstacle chunks while the batch is at most one instance per CU, else one; 1; 4
    bool dynamic_rows = true;     // QP kernel as a persistent launch whose rows pull instances from a queue (0: one group per row for the whole launch)
    int handover_iter = -1;       // IPM iterations after which a row of a drained launch hands its instance to the follow-up launch (0: never; -1: qp_plan.hpp decides)
    bool handover_lds = true;     // the follow-up launch copies the planes into LDS when the horizon fits
    int handover_co = -1;         // the follow-up kernel beside the draining launch (usv_qp_resume_co): -1 when the follow-up works in LDS, 0 never, 1 the same
    int co_spin_limit = 200000;   // polls of ~1 us a co-resident workgroup waits for its entry before it gives up
    long co_wgs = 0;              // workgroups of the co-resident launch (0: one per CU - qp_plan.hpp says why)
    unsigned noise_mask = ~0u;    // states usvmpc_advance disturbs (bit j: state j)
    long long instance_offset = 0; // global index of the handle's first instance: keys the disturbance (a shard draws what the unsharded batch draws)
    bool merge_rows = true;       // box rows processed in their slot lanes when all of them ride there (another set of kernels: qp_ipm.hpp, MERGE)
    bool step_on_advance = true;  // usvmpc_advance / _advance_sim move the world too (obstacle tracks and the path-following front end's)
    bool pf_predict = true;       // a moving world of the path-following front end: 1 predicted per stage, 0 held still inside the horizon (stage 0 only, "static_obstacles" on)
    double pf_margin = 0.2;       // the path-following front end's lh = (R + boat radius) + margin (scripts/usv_pf_ca/main.py:126)
    int cond_N2 = 0;              // partial condensing: RTI solves condense the QP to cond_N2 stages first (0: off - the Riccati sweep over the N stages)
    bool tracks_on = false;       // p is derived from the obstacle tracks (usv_obstacle_predict before every solve that needs it)

    static Options defaults(bool model_has_pairs)
    {
        Options o;
        o.lin_pairs = model_has_pairs ? 1 : 0;
        return o;
    }
};

// a member of Options as a table entry: its type and place
struct OptMember {
    enum Type { NONE, BOOL, INT, LONG, UNSIGNED, LLONG, DOUBLE } type;
    size_t off;
};
constexpr OptMember::Type opt_type(const bool *) { return OptMember::BOOL; }
constexpr OptMember::Type opt_type(const int *) { return OptMember::INT; }
constexpr OptMember::Type opt_type(const long *) { return OptMember::LONG; }
constexpr OptMember::Type opt_type(const unsigned *) { return OptMember::UNSIGNED; }
constexpr OptMember::Type opt_type(const long long *) { return OptMember::LLONG; }
constexpr OptMember::Type opt_type(const double *) { return OptMember::DOUBLE; }
#define USV_OPT_AT(m) OptMember{opt_type((const decltype(Options::m) *)nullptr), offsetof(Options, m)}
constexpr OptMember OPT_NOWHERE = {OptMember::NONE, 0};

// a normalised value (parse_option) into / out of its member; every normalised value is a whole number its member's type holds, or a double
inline void store(Options &o, OptMember at, double v)
{
    char *p = reinterpret_cast<char *>(&o) + at.off;
    switch (at.type) {
    case OptMember::NONE: break;
    case OptMember::BOOL: *reinterpret_cast<bool *>(p) = v != 0.0; break;
    case OptMember::INT: *reinterpret_cast<int *>(p) = (int)v; break;
    case OptMember::LONG: *reinterpret_cast<long *>(p) = (long)v; break;
    case OptMember::UNSIGNED: *reinterpret_cast<unsigned *>(p) = (unsigned)v; break;
    case OptMember::LLONG: *reinterpret_cast<long long *>(p) = (long long)v; break;
    case OptMember::DOUBLE: *reinterpret_cast<double *>(p) = v; break;
    }
}
inline double load(const Options &o, OptMember at)
{
    const char *p = reinterpret_cast<const char *>(&o) + at.off;
    switch (at.type) {
    case OptMember::NONE: break;
    case OptMember::BOOL: return *reinterpret_cast<const bool *>(p);
    case OptMember::INT: return *reinterpret_cast<const int *>(p);
    case OptMember::LONG: return (double)*reinterpret_cast<const long *>(p);
    case OptMember::UNSIGNED: return *reinterpret_cast<const unsigned *>(p);
    case OptMember::LLONG: return (double)*reinterpret_cast<const long long *>(p);
    case OptMember::DOUBLE: return *reinterpret_cast<const double *>(p);
    }
    return 0.0;
}

// ---- 2. the table
enum OptId {
    OPT_OBSTACLE_TRACKS = 0, OPT_OBSTACLE_STEP_ON_ADVANCE, OPT_PF_PREDICT, OPT_PF_LH_MARGIN, OPT_PIPELINE_LINEARIZE, OPT_SORT_TWO_TICKS,
    OPT_SORT_BY_DIFFICULTY, OPT_MAX_WAVES, OPT_KEEP_MULTIPLIERS, OPT_QP_COND_N, OPT_LIN_FORCE_MODES, OPT_LIN_PAIRS, OPT_AUX_IN_LDS,
    OPT_DYNAMIC_ROWS, OPT_HANDOVER_LDS, OPT_MERGE_BOX_ROWS, OPT_LDS_WORKSPACE, OPT_WIDE, OPT_WIDE_WAVES, OPT_COND_PRED_CORR, OPT_CPC_FACTOR,
    OPT_HPIPM_MODE, OPT_HANDOVER_ITER, OPT_HANDOVER_CO, OPT_HANDOVER_CO_SPIN, OPT_HANDOVER_CO_WGS, OPT_DISTURBANCE_MASK, OPT_INSTANCE_OFFSET,
    OPT_HOST_MIRROR, OPT_STATIC_OBSTACLES, OPT_PACK_BOX_ROWS, OPT_COUNT
};
enum OptKind { // the caller's double v -> the normalised value; [lo, hi] are the row's bounds on v (a NaN lies in no range)
    K_FLAG,       // v != 0
    K_SIGN,       // v < 0: -1; v > 0: 1; else 0
    K_SIGN_NZ,    // v < 0: -1; v != 0: 1; else 0
    K_WAVES,      // v < 0: -1; v >= 4: 4; else 1
    K_REAL,       // v, refused outside [lo, hi]
    K_WHOLE,      // v, refused outside [lo, hi] or with a fraction
    K_TRUNC,      // v truncated towards 0, refused outside [lo, hi]
    K_TRUNC_NEG1  // v < 0: -1; else as K_TRUNC
};
enum : unsigned { // effects: what usvmpc.hip's apply_option does beside the store, in this order
    FX_KEEPS_AHEAD = 1,  // a linearisation made a tick ahead stays good (no spec_cancel): the option touches nothing a lineariser reads or is ordered by
    FX_IF_CHANGED = 2,   // the effects below apply only when the stored value changes
    FX_CAPS = 4,         // the occupancy answers are dropped (QpCaps::reset): another kernel, grid or LDS size may be launched
    FX_COND_RELEASE = 8, // the condensing buffers are released (sized for the old value: launch_cond makes them anew)
    FX_MAP_CHANGED = 16, // the workspace's multipliers no longer belong to the solve that comes next (usvmpc_handle::map_changed)
    FX_LAYOUT_DIRTY = 32, // the row layout changed: the workspace cannot be read back before the next solve
    FX_TRACKS_DIRTY = 64, // p on the device is not what the obstacle tracks predict (the stages the prediction writes change)
    FX_UPLOAD_SPEC = 128, // DevSpec goes up to the device
    FX_HOOK = 256         // more in usvmpc.hip that needs HIP or other handle state: option_refused (before anything is done), option_hook (last)
};

struct OptRow {
    const char *name;
    OptId id;
    OptKind kind;
    double lo, hi;
    const char *refusal; // the text when the kind refuses
    OptMember at;
    unsigned fx;
};

constexpr double D_INF = std::numeric_limits<double>::infinity(), D_MAX = std::numeric_limits<double>::max();
// the open ends of the ranges whose every value converts: the smallest double above -1 and the largest below 2^32 (unsigned) / 2^63 (long)
constexpr double ABOVE_M1 = -0x1.fffffffffffffp-1, BELOW_2P32 = 0x1.fffffffffffffp+31, BELOW_2P63 = 0x1.fffffffffffffp+62;
static_assert(ABOVE_M1 > -1.0 && BELOW_2P32 < 4294967296.0 && BELOW_2P63 < 9223372036854775808.0, "inside the open ranges");
static_assert(sizeof(long) == 8 && sizeof(unsigned) == 4 && sizeof(int) == 4, "the ranges below are those of these types");

constexpr OptRow OPTION_TABLE[OPT_COUNT] = {
    // name                        id                            kind          lo        hi          refusal                                            member                       effects
    // (the first four: p, lh and the world are read by no lineariser)
    {"obstacle_tracks",          OPT_OBSTACLE_TRACKS,          K_WHOLE,      0,        1,          "obstacle_tracks: 0 or 1",                         USV_OPT_AT(tracks_on),       FX_KEEPS_AHEAD | FX_HOOK}, // (hook: who owns p; on: tracks dirty)
    {"obstacle_step_on_advance", OPT_OBSTACLE_STEP_ON_ADVANCE, K_FLAG,       0,        0,          nullptr,                                           USV_OPT_AT(step_on_advance), FX_KEEPS_AHEAD},
    {"pf_predict",               OPT_PF_PREDICT,               K_WHOLE,      0,        1,          "pf_predict: 0 or 1",                              USV_OPT_AT(pf_predict),      FX_KEEPS_AHEAD | FX_HOOK}, // (hook: "static_obstacles" as the front end then needs it)
    {"pf_lh_margin",             OPT_PF_LH_MARGIN,             K_REAL,       0,        D_MAX,      "pf_lh_margin must be finite and non-negative",    USV_OPT_AT(pf_margin),       FX_KEEPS_AHEAD},
    {"pipeline_linearize",       OPT_PIPELINE_LINEARIZE,       K_FLAG,       0,        0,          nullptr,                                           USV_OPT_AT(pipeline),        0},
    {"sort_two_ticks",           OPT_SORT_TWO_TICKS,           K_FLAG,       0,        0,          nullptr,                                           USV_OPT_AT(sort_two),        0},
    {"sort_by_difficulty",       OPT_SORT_BY_DIFFICULTY,       K_FLAG,       0,        0,          nullptr,                                           USV_OPT_AT(sort_enabled),    FX_HOOK}, // (hook: off while a map is set - the map is dropped, map changed)
    {"max_waves",                OPT_MAX_WAVES,                K_TRUNC,      -0x1p+63, BELOW_2P63, "max_waves out of range",                          USV_OPT_AT(max_waves),       FX_CAPS | FX_COND_RELEASE},
    {"keep_multipliers",         OPT_KEEP_MULTIPLIERS,         K_FLAG,       0,        0,          nullptr,                                           OPT_NOWHERE,                 FX_HOOK}, // (an action: the hook makes the "lam" / "t" buffers)
    // (0 and N both mean off: parse_option, which also checks the sizes)
    {"qp_cond_N",                OPT_QP_COND_N,                K_TRUNC,      ABOVE_M1, D_INF,      "qp_cond_N must lie in 0..N",                      USV_OPT_AT(cond_N2),         FX_IF_CHANGED | FX_COND_RELEASE | FX_MAP_CHANGED},
    {"lin_force_modes",          OPT_LIN_FORCE_MODES,          K_WHOLE,      0,        2,          "lin_force_modes: 0, 1 or 2",                      USV_OPT_AT(lin_force),       0},
    {"lin_pairs",                OPT_LIN_PAIRS,                K_WHOLE,      0,        1,          "lin_pairs: 0 or 1",                               USV_OPT_AT(lin_pairs),       0},
    {"aux_in_lds",               OPT_AUX_IN_LDS,               K_FLAG,       0,        0,          nullptr,                                           USV_OPT_AT(aux_lds),         FX_CAPS},
    {"dynamic_rows",             OPT_DYNAMIC_ROWS,             K_FLAG,       0,        0,          nullptr,                                           USV_OPT_AT(dynamic_rows),    FX_CAPS},
    {"handover_lds",             OPT_HANDOVER_LDS,             K_FLAG,       0,        0,          nullptr,                                           USV_OPT_AT(handover_lds),    FX_CAPS},
    {"merge_box_rows",           OPT_MERGE_BOX_ROWS,           K_FLAG,       0,        0,          nullptr,                                           USV_OPT_AT(merge_rows),      FX_CAPS}, // (another set of kernels: merged / two-pass instantiations, wide ones included)
    {"lds_workspace",            OPT_LDS_WORKSPACE,            K_SIGN,       0,        0,          nullptr,                                           USV_OPT_AT(lds_mode),        FX_CAPS},
    {"wide",                     OPT_WIDE,                     K_SIGN,       0,        0,          nullptr,                                           USV_OPT_AT(wide_mode),       FX_CAPS},
    {"wide_waves",               OPT_WIDE_WAVES,               K_WAVES,      0,        0,          nullptr,                                           USV_OPT_AT(wide_waves),      FX_CAPS},
    // HPIPM's conditional predictor-corrector (d_ocp_qp_ipm_arg.cond_pred_corr: on in every mode acados picks from - DESIGN.md section 2): a
    // corrected step that leaves the duality measure above cpc_factor (2) x the predictor's mu_aff is replaced by the centring-only step.
    // Changes the iteration path, i.e. results inside the exit tolerance ball.  Built into every kernel; the option switches the test.
    // "hpipm_mode": the profile's values of mu0, alpha_min and cond_pred_corr (host_spec.hpp, hpipm_profile).
    {"cond_pred_corr",           OPT_COND_PRED_CORR,           K_FLAG,       0,        0,          nullptr,                                           OPT_NOWHERE,                 FX_UPLOAD_SPEC},
    {"cpc_factor",               OPT_CPC_FACTOR,               K_REAL,       std::numeric_limits<double>::denorm_min(), D_INF, "cpc_factor must be positive", OPT_NOWHERE,          FX_UPLOAD_SPEC}, // (v > 0)
    {"hpipm_mode",               OPT_HPIPM_MODE,               K_WHOLE,      USVMPC_HPIPM_BALANCE, USVMPC_HPIPM_R04, "hpipm_mode must be one of USVMPC_HPIPM_*", OPT_NOWHERE,       FX_UPLOAD_SPEC},
    {"handover_iter",            OPT_HANDOVER_ITER,            K_TRUNC_NEG1, -D_INF,   1e6,        "handover_iter out of range",                      USV_OPT_AT(handover_iter),   0},
    {"handover_co",              OPT_HANDOVER_CO,              K_SIGN_NZ,    0,        0,          nullptr,                                           USV_OPT_AT(handover_co),     0},
    {"handover_co_spin",         OPT_HANDOVER_CO_SPIN,         K_TRUNC,      1,        2e9,        "handover_co_spin out of range",                   USV_OPT_AT(co_spin_limit),   0},
    {"handover_co_wgs",          OPT_HANDOVER_CO_WGS,          K_TRUNC,      0,        1e6,        "handover_co_wgs out of range",                    USV_OPT_AT(co_wgs),          0},
    {"disturbance_mask",         OPT_DISTURBANCE_MASK,         K_TRUNC,      ABOVE_M1, BELOW_2P32, "disturbance_mask out of range",                   USV_OPT_AT(noise_mask),      0},
    {"instance_offset",          OPT_INSTANCE_OFFSET,          K_WHOLE,      0,        0x1p+53,    "instance_offset must be a non-negative integer",  USV_OPT_AT(instance_offset), 0},
    {"host_mirror",              OPT_HOST_MIRROR,              K_FLAG,       0,        0,          nullptr,                                           OPT_NOWHERE,                 FX_HOOK}, // (0: the hook flushes the mirror and gives it up; it does not come back)
    {"static_obstacles",         OPT_STATIC_OBSTACLES,         K_FLAG,       0,        0,          nullptr,                                           OPT_NOWHERE,                 FX_TRACKS_DIRTY | FX_UPLOAD_SPEC},
    {"pack_box_rows",            OPT_PACK_BOX_ROWS,            K_FLAG,       0,        0,          nullptr,                                           OPT_NOWHERE,                 FX_CAPS | FX_LAYOUT_DIRTY | FX_UPLOAD_SPEC}, // (on only where the rows fit: parse_option)
};

constexpr bool same_name(const char *a, const char *b)
{
    for (; *a && *a == *b; a++, b++) {}
    return *a == *b;
}
constexpr bool option_table_sound()
{
    for (int i = 0; i < OPT_COUNT; i++) {
        if (OPTION_TABLE[i].id != i) return false;
        for (int j = 0; j < i; j++)
            if (same_name(OPTION_TABLE[i].name, OPTION_TABLE[j].name)) return false;
    }
    return true;
}
static_assert(option_table_sound(), "OPTION_TABLE[id] is the row of id, and no name comes twice");

// the row of a name; nullptr: no such option (a null name included)
inline const OptRow *find_option(const char *name)
{
    if (name)
        for (const OptRow &r : OPTION_TABLE)
            if (same_name(r.name, name)) return &r;
    return nullptr;
}

// ---- 3. a call of usvmpc_set_option, as far as it can be judged without the handle
struct OptFacts { // the handle's sizes and what its model and layout allow
    int N, nx, nu, K;
    bool has_pairs;  // the model declares the columns the paired lineariser integrates (PairCols)
    bool any_bsoft;  // DevSpec::any_bsoft: soft state bounds
    bool boxpack_ok; // DevSpec::boxpack_ok: the box rows fit the obstacle rows' planes
};
struct OptParse {
    const OptRow *row; // nullptr: unknown
    double value;      // normalised
    int rc;            // 0, USVMPC_E_ARG (refused) or USVMPC_E_FIELD (unknown name)
    std::string err;
};

inline OptParse parse_option(const char *name, double v, const OptFacts &f)
{
    const OptRow *row = find_option(name);
    if (!row) return OptParse{nullptr, 0.0, USVMPC_E_FIELD, std::string("unknown option '") + (name ? name : "") + "'"};
    auto refuse = [row](const char *why) { return OptParse{row, 0.0, USVMPC_E_ARG, why}; };
    const bool inside = v >= row->lo && v <= row->hi;
    double out = v;
    switch (row->kind) {
    case K_FLAG: out = v != 0.0 ? 1 : 0; break;
    case K_SIGN: out = v < 0.0 ? -1 : (v > 0.0 ? 1 : 0); break;
    case K_SIGN_NZ: out = v < 0.0 ? -1 : (v != 0.0 ? 1 : 0); break;
    case K_WAVES: out = v < 0.0 ? -1 : (v >= 4.0 ? 4 : 1); break;
    case K_REAL: if (!inside) return refuse(row->refusal); break;
    case K_WHOLE: if (!inside || v != std::trunc(v)) return refuse(row->refusal); break;
    case K_TRUNC: if (!inside) return refuse(row->refusal); out = std::trunc(v); break;
    case K_TRUNC_NEG1: if (!inside) return refuse(row->refusal); out = v < 0.0 ? -1 : std::trunc(v); break;
    }
    switch (row->id) { // what depends on the handle's sizes
    case OPT_OBSTACLE_TRACKS:
        if (out != 0.0 && f.K == 0) return refuse("obstacle_tracks: this model has no obstacle rows (K = 0)");
        break;
    case OPT_QP_COND_N: // acados qp_solver_cond_N: stages of the partially condensed QP; 0 or N: no condensing
        if (out > f.N) return refuse(row->refusal);
        if (out == f.N) out = 0;
        if (out > 0) {
            // (blocks as HPIPM partitions them: N / N2 stages each, the first N mod N2 one more; one block's variables must fit a wave)
            const int n2 = (int)out;
            if (f.nx + ((f.N + n2 - 1) / n2) * f.nu > 64) return refuse("qp_cond_N: a condensed stage may have at most 64 variables (nx + ceil(N / qp_cond_N) nu)");
            if (f.any_bsoft) return refuse("partial condensing (qp_cond_N) is not built for soft state bounds");
        }
        break;
    case OPT_LIN_PAIRS:
        if (out != 0.0 && !f.has_pairs) return refuse("lin_pairs: the model does not declare the columns to integrate");
        break;
    case OPT_PACK_BOX_ROWS:
        if (!f.boxpack_ok) out = 0;
        break;
    default: break;
    }
    return OptParse{row, out + 0.0, 0, std::string()}; // (+ 0.0: a -0.0 that came through is 0)
}

} // namespace usv
