// qp_plan.hpp — how a batch of QPs is mapped onto the device: a pure host function from numbers (the handle's sizes and options, the
// facts of its kernel table, what the occupancy queries said) to the launches of one solve.  No HIP header: usvmpc.hip's launch_qp fills
// QpIn, answers the queries and carries the plan out; tests/qp_plan_harness.cpp does the same with a device made of numbers.
#pragma once

#include <algorithm>
#include <cstddef>

namespace usv {

// The QP kernels of the table (Kernels::qp in usvmpc.hip is indexed by the first seven); the follow-up kernels of a hand-over have another
// signature and appear here for the occupancy queries only.
enum QpSlot {
    SLOT_QP = 0,     // four instances per wave: planes in HBM
    SLOT_QP_LDS,     // ... the workspace in LDS
    SLOT_QP_AUX,     // ... the aux plane in LDS
    SLOT_WIDE_LDS1,  // the latency mapping: [planes in LDS, in HBM] x [one wave, four waves per instance]
    SLOT_WIDE_HBM1,
    SLOT_WIDE_LDS4,
    SLOT_WIDE_HBM4,
    SLOT_QP_KERNELS,
    SLOT_RESUME = SLOT_QP_KERNELS, // the follow-up launch of a hand-over: over the planes in HBM
    SLOT_RESUME_LDS,               // ... after copying them into LDS
    SLOT_COUNT
};

constexpr long CU_LDS_BYTES = 160L * 1024; // LDS of a CU: a kernel's static and dynamic LDS come out of it
constexpr long WINDOW_LIMIT = 1L << 32;    // a buffer window is addressed with 32-bit offsets
constexpr int PLANE_ROW_BYTES = 128;       // one group's row of a workspace plane: 16 lanes of FP64
constexpr int QP_BLOCK = 64;               // threads of a QP workgroup: one wave (the four-wave mapping: four)
constexpr int QP_GROUP_LANES = 16;         // lanes of a group (params.hpp LANES)

// What the occupancy queries said about the handle's kernels - 0: not yet known, -1: does not fit, n otherwise.  Whatever changes WHICH
// kernel a launch takes (row layout, mapping, wave cap, workspace placement) calls reset(): plan_qp then asks again - for every kernel
// of the handle's table.
struct QpCaps {
    long qp;                // groups a full-occupancy launch of the QP kernel holds at once
    long lds;               // waves an LDS-workspace launch holds at once
    long aux;               // as qp, for the aux-in-LDS instantiation (-1: does not fit / would cost a wave)
    long wide;              // waves a launch of the wide kernel holds at once
    long wide_hbm;          // the same for the wide kernel over planes in HBM (horizons that do not fit LDS)
    long wide4, wide4_hbm;  // workgroups of four waves a launch holds at once
    long resume;            // workgroups of the follow-up launch (-1: the kernel cannot be launched)
    bool resume_lds;        // the follow-up launch copies the planes into LDS (chosen with resume)
    long lds_static;        // static LDS of SLOT_QP_LDS, bytes - a constant of the code object (-1: not yet asked)
    void reset()
    {
        qp = 0; lds = 0; aux = 0; wide = 0; wide_hbm = 0; wide4 = 0; wide4_hbm = 0; resume = 0;
        resume_lds = false; lds_static = -1;
    }
};

struct QpIn {
    // the handle: sizes, the row layout's planes, the launch
    int B, Bp, N, K;
    int npt, nu, aux_dense4;  // DevSpec::npt, the model's nu, DevSpec::aux_dense4
    int kch;                  // the handle's obstacle chunks
    int phase;                // 0: an RTI solve; 1, 2: the launches of a full SQP
    int ncu;
    // options
    int wide_mode, wide_waves, lds_mode;
    bool dynamic_rows;
    long max_waves;
    bool aux_lds;
    int handover_iter;
    bool handover_lds;
    int handover_co;
    long co_wgs;
    bool own_stream;
    // the kernel table
    bool has[SLOT_COUNT];     // the kernel exists for the row layout
    bool has_resume_co;
    int nplw, ex_lds, ex_hbm; // planes per stage an instance keeps in LDS; planes of the exchange area (qp_ipm.hpp NPLW, EX_N)
    int k_kch;                // the instantiation's KCH and SOFT (kch and the handle's soft may differ: usv_model with "soft" set)
    bool k_soft;
};

struct QpPlan {
    // the main launch: kernel<<<grid, block, lds_bytes>>>(ptrs, ngroups, phase, q0, rows)
    QpSlot slot;
    long grid;
    int block;
    size_t lds_bytes;
    long ngroups;
    int q0;                   // first group the queue hands out (-1: no queue, the queue word is left alone)
    int rows;
    int mapping;              // waves per instance of the latency mapping, 0: the throughput mapping (usvmpc_last_mapping)
    // the hand-over of long runners
    bool hand_ready;          // the follow-up kernel can be launched: its buffers are wanted, handed over or not
    bool hand;                // rows hand over past hand_iter iterations; the follow-up launch goes behind the main one
    bool hand_lds;            // ... with the planes copied into LDS (SLOT_RESUME_LDS), else over the planes in HBM (SLOT_RESUME)
    size_t hand_bytes;        // dynamic LDS of the follow-up kernels
    int hand_iter;
    long hand_wgs;
    // the follow-up kernel beside the draining launch
    bool co;                  // wanted (the executor still has to make its stream: co_prepare)
    long co_wgs;
};

// One workgroup per instance; with the queue at most `cap` of them, which pull the remaining instances as theirs finish.
inline void plan_per_instance(QpPlan &p, QpSlot slot, int block, size_t bytes, long B, long cap, bool queue, int mapping)
{
    long nw = B;
    int q0 = -1;
    if (queue && nw > cap) { nw = cap; q0 = (int)nw; }
    p.slot = slot; p.grid = nw; p.block = block; p.lds_bytes = bytes;
    p.ngroups = nw; p.q0 = q0; p.rows = 1;
    p.mapping = mapping;
}

// Probe: int blocks(QpSlot, int block, size_t dyn) - workgroups of `block` threads a CU holds of the kernel with `dyn` bytes of dynamic
// LDS, 0: it does not fit; long static_lds(QpSlot) - the kernel's static LDS.  Asked only for kernels that exist, only when the answer
// decides something, and once: the answers are kept in `c`.
//
// An RTI solve is ONE launch of as many waves as the device holds at once; their rows start on the first groups and
// pull the remaining ones from a queue as they finish (qp_ipm.hpp).  The full SQP keeps one group per row: its later
// iterations find their multipliers in the group's part of the workspace.
// Small batches: the planes of every instance in flight fit in LDS (160 KB per CU), and a solve whose sweeps wait for
// HBM at every stage - nothing else runs on the CU to hide it - becomes a solve on LDS.  rows_lds instances per wave
// (as many whole horizons as fit), one wave per CU at a time; further instances come through the same queue.
template <class Probe>
QpPlan plan_qp(const QpIn &in, QpCaps &c, Probe &&probe)
{
    QpPlan p = {};
    const long B = in.B, ncu = in.ncu;
    const int phase = in.phase;
    const size_t planes_lds = (size_t)(in.N + 1) * (size_t)in.nplw * PLANE_ROW_BYTES; // an instance's planes in LDS
    // the window of a block of `stages` stages (32-bit offsets)
    auto window = [&in](int stages) { return (long)std::min(in.N + 1, stages) * in.Bp * in.npt * PLANE_ROW_BYTES; };
    // Four waves per instance (qp_ipm.hpp, WW): a workgroup = a whole CU shares out the row work of 16 consecutive stages - for the
    // single instance and batches of at most one instance per CU.
    if (in.has[SLOT_WIDE_LDS4] && phase == 0 && in.wide_mode != 0 && in.wide_waves != 1 && ncu > 0) {
        // (the exchange area of 16 stages and one row more that the four waves share: qp_ipm.hpp wide_lds_doubles)
        const size_t b4 = planes_lds + (size_t)16 * in.ex_lds * PLANE_ROW_BYTES + PLANE_ROW_BYTES, x4 = (size_t)16 * in.ex_hbm * PLANE_ROW_BYTES + PLANE_ROW_BYTES;
        if (c.wide4 == 0) c.wide4 = probe.blocks(SLOT_WIDE_LDS4, 4 * QP_BLOCK, b4) > 0 ? ncu : -1;
        if (c.wide4 < 0 && c.wide4_hbm == 0)
            c.wide4_hbm = (window(16) < WINDOW_LIMIT && in.has[SLOT_WIDE_HBM4] && probe.blocks(SLOT_WIDE_HBM4, 4 * QP_BLOCK, x4) > 0) ? ncu : -1;
        const bool lds = c.wide4 > 0;
        long cap = lds ? c.wide4 : c.wide4_hbm;
        if (cap > 0 && in.max_waves > 0) cap = std::max<long>(1, std::min(cap, in.max_waves / 4)); // option "max_waves" counts wavefronts
        // default: where the row work is the larger share - the soft-row OCPs and two obstacle chunks (measured, one instance / 256 instances
        // per tick: usv_model_guidance_ca1 N = 100 / K = 8 1.78 -> 1.59 / 5.6 -> 5.0 ms, N = 40 / K = 10 0.94 -> 0.86 / 2.05 -> 1.87, N = 80 / K = 20
        // 4.00 -> 3.00 / 8.1 -> 6.2; usv_model_pf_ca N = 80 / K = 20 6.95 -> 6.22 / 10.4 -> 9.6, with ONE chunk of hard rows 0 - 7 % SLOWER: there
        // the recursion dominates and pays the barriers)
        // Up to one instance per CU; with the queue and a horizon of 40 or more up to two (tools/latency_probe.py over 13 shapes x 7 batch sizes,
        // profiles/r05_f_policy_audit.txt: 512 instances 6 - 8 % under one wave each; at N = 20 the second round costs more than the row work saves)
        const long reach = (in.dynamic_rows && in.N >= 40) ? 2 * cap : cap;
        // (round 6, profiles/r06_b_policy_audit.txt: ONE chunk of hard rows also gains 2 - 4 % from four waves when the rows are many and the
        // horizon long - usv_model_pf_ca N = 40 / K = 10: one instance 2.50 -> 2.40 ms, 64: 5.84 -> 5.63, 256: 4.03 -> 3.94; N = 100 / K = 8,
        // 64: 9.62 -> 9.34; with K = 3 or 4 it loses - up to one instance per CU)
        const bool hard_many = !in.k_soft && in.k_kch == 1 && in.K >= 8 && in.N >= 40 && B <= cap;
        if (cap > 0 && (in.wide_waves == 4 || ((in.k_soft || in.k_kch == 2) && B <= reach) || hard_many)) {
            plan_per_instance(p, lds ? SLOT_WIDE_LDS4 : SLOT_WIDE_HBM4, 4 * QP_BLOCK, lds ? b4 : x4, B, cap, in.dynamic_rows, 4);
            return p;
        }
    }
    // The latency mapping: ONE instance per wave (qp_ipm.hpp, WIDE) - planes in LDS, the four rows share out the stage-local row
    // work.  A wave then finishes an instance 1.4x (hard rows) to 1.8x (soft rows) sooner and the device holds a quarter of the instances at once: it pays while
    // the batch leaves SIMDs idle anyway (a solve of the batch then lasts as long as its hardest instance on a lone wave).
    if (in.has[SLOT_WIDE_LDS1] && in.wide_mode != 0 && ncu > 0) {
        if (phase == 0) { // (the launches of a full SQP find their multipliers in the group's planes in HBM: the variant over planes in HBM below)
            // (in LDS: the planes the solve writes - WsLayout's up to L_zu less the four box planes the packed layouts leave unused)
            const size_t bytes = planes_lds + (size_t)4 * in.ex_lds * PLANE_ROW_BYTES;
            if (c.wide == 0) {
                const int nb = probe.blocks(SLOT_WIDE_LDS1, QP_BLOCK, bytes);
                c.wide = nb > 0 ? (long)std::min(nb, 4) * ncu : -1; // (one wave per SIMD at most: the point is a lone wave's issue rate)
                if (c.wide > 0 && in.max_waves > 0) c.wide = std::min(c.wide, in.max_waves); // option "max_waves"
            }
            // default: while the batch fits the SIMDs twice over (the queue hands the second half to the waves that finish first)
            if (c.wide > 0 && (in.wide_mode > 0 || B <= 2 * c.wide)) {
                // (without the queue every instance needs its wave at launch: still correct, later workgroups wait)
                plan_per_instance(p, SLOT_WIDE_LDS1, QP_BLOCK, bytes, B, c.wide, in.dynamic_rows, 1);
                return p;
            }
        }
        // The horizon's planes do not fit a CU's LDS (the reference node's own N = 100: nmpc_guidance_ca1.cpp:64), or the launch belongs to a
        // full SQP: the same sweeps over the planes in HBM / L2 - the four rows of a wave address the four stages of a block through one
        // window, the next block's row planes and the next stage's recursion planes are in flight ahead of their use.
        if ((c.wide < 0 || phase != 0) && in.has[SLOT_WIDE_HBM1] && window(4) < WINDOW_LIMIT) {
            const size_t xbytes = (size_t)4 * in.ex_hbm * PLANE_ROW_BYTES;
            if (c.wide_hbm == 0) {
                const int nb = probe.blocks(SLOT_WIDE_HBM1, QP_BLOCK, xbytes);
                c.wide_hbm = nb > 0 ? (long)std::min(nb, 4) * ncu : -1;
                if (c.wide_hbm > 0 && in.max_waves > 0) c.wide_hbm = std::min(c.wide_hbm, in.max_waves);
            }
            // default: an RTI solve while the batch fits the resident waves twice over, as with the planes in LDS (measured at 2 048 instances, N = 80 / 100:
            // 1.2 - 1.3x the throughput mapping; at 4 096 the throughput mapping is ahead); the launches of a full SQP once (no queue there)
            const long reach = (phase == 0 && in.dynamic_rows) ? 2 * c.wide_hbm : c.wide_hbm;
            if (c.wide_hbm > 0 && (in.wide_mode > 0 || B <= reach)) {
                // (full SQP: one group per workgroup for the whole call - its multipliers persist in the group's planes)
                plan_per_instance(p, SLOT_WIDE_HBM1, QP_BLOCK, xbytes, B, c.wide_hbm, in.dynamic_rows && phase == 0, 1);
                return p;
            }
        }
    }
    // (the kernel's own static LDS - exchange area, parked constants - comes out of the same 160 KB)
    if (in.has[SLOT_QP_LDS] && c.lds_static < 0) c.lds_static = probe.static_lds(SLOT_QP_LDS);
    const long lds_inst = (long)(in.N + 1) * in.npt * PLANE_ROW_BYTES;
    const int rows_lds = (int)std::min<long>(4, (CU_LDS_BYTES - (in.has[SLOT_QP_LDS] ? c.lds_static : 0)) / lds_inst);
    bool use_lds = phase == 0 && in.lds_mode != 0 && in.has[SLOT_QP_LDS] && rows_lds >= 1 && ncu > 0;
    // by default only while one round of workgroups covers the batch: measured on usv_model_pf_ca, N = 20 / K = 3, the solve
    // of 512 instances takes 5.9 ms with the planes in LDS against 6.5 ms in HBM, at 1024 (two rounds) 7.5 against 7.1
    if (use_lds && in.lds_mode < 0) use_lds = B <= (long)rows_lds * ncu;
    if (use_lds) {
        const size_t bytes = (size_t)rows_lds * lds_inst;
        if (c.lds == 0) {
            const int nb = probe.blocks(SLOT_QP_LDS, QP_BLOCK, bytes);
            c.lds = nb > 0 ? (long)nb * ncu : -1;
        }
        if (c.lds > 0) {
            long nw = (B + rows_lds - 1) / rows_lds;
            int q0 = -1;
            if (in.dynamic_rows && nw > c.lds) { nw = c.lds; q0 = (int)(nw * rows_lds); }
            p.slot = SLOT_QP_LDS; p.grid = nw; p.block = QP_BLOCK; p.lds_bytes = bytes;
            p.ngroups = nw * rows_lds; p.q0 = q0; p.rows = rows_lds;
            return p;
        }
    }
    // The throughput mapping: four instances per wave, one group per row
    long ng = in.Bp;
    int q0 = -1;
    if (in.dynamic_rows && phase == 0 && c.qp == 0) {
        const int nb = probe.blocks(SLOT_QP, QP_BLOCK, 0);
        c.qp = (nb > 0 && ncu > 0) ? 4L * nb * ncu : -1;
    }
    // The aux plane in LDS (qp_ipm.hpp, AUXLDS): 4 rows x (N + 1) stages x at most ten values beside the kernel's static LDS - taken
    // when it does not cost a resident wave (usv_model_pf_ca at N = 40, K = 10: 13.1 KB + 6.7 KB of the 20 KB a wave may have)
    size_t aux_bytes = 0;
    if (phase == 0 && in.has[SLOT_QP_AUX] && in.aux_lds && in.dynamic_rows && c.qp > 0) {
        aux_bytes = (size_t)4 * (in.N + 1) * (size_t)(in.aux_dense4 + (in.kch > 0 ? 2 : 0) + 2 * in.nu) * sizeof(double);
        if (c.aux == 0) {
            const long cap = 4L * probe.blocks(SLOT_QP_AUX, QP_BLOCK, aux_bytes) * ncu;
            c.aux = cap >= c.qp ? cap : -1;
        }
        if (c.aux < 0) aux_bytes = 0;
    }
    if (in.dynamic_rows && phase == 0) {
        long cap = aux_bytes ? std::min(c.aux, c.qp) : c.qp;
        if (in.max_waves > 0 && 4L * in.max_waves < cap) cap = 4L * in.max_waves; // option "max_waves": fewer resident waves
        if (cap > 0 && cap < ng) { ng = cap; q0 = (int)ng; }
    }
    p.slot = aux_bytes ? SLOT_QP_AUX : SLOT_QP;
    p.grid = (ng * QP_GROUP_LANES + QP_BLOCK - 1) / QP_BLOCK; p.block = QP_BLOCK; p.lds_bytes = aux_bytes;
    p.ngroups = ng; p.q0 = q0; p.rows = 4;
    // Hand-over of long runners (qp_ipm.hpp, QpIpm::suspend): a launch that refills from the queue ends with a few rows finishing
    // instances of 30 - 50 iterations on an idling device; past "handover_iter" iterations those go to a follow-up launch on the
    // latency mapping (one instance per wave over the same planes: 1.6x per pass for usv_model_pf_ca at N = 40).  Scheduling only.
    if (phase == 0 && in.handover_iter != 0 && in.has[SLOT_RESUME] && window(4) < WINDOW_LIMIT) {
        const size_t xbytes = (size_t)4 * in.ex_hbm * PLANE_ROW_BYTES;
        const size_t lbytes = planes_lds + (size_t)4 * in.ex_lds * PLANE_ROW_BYTES;
        if (c.resume == 0) {
            // (planes in LDS when the horizon fits - option "handover_lds", default on -, else over the planes in HBM)
            const int nb_lds = (in.handover_lds && ncu > 0 && in.has[SLOT_RESUME_LDS]) ? probe.blocks(SLOT_RESUME_LDS, QP_BLOCK, lbytes) : 0;
            const int nb = nb_lds > 0 ? nb_lds : probe.blocks(SLOT_RESUME, QP_BLOCK, xbytes);
            c.resume_lds = nb_lds > 0;
            c.resume = (nb > 0 && ncu > 0) ? (long)std::min(nb, 4) * ncu : -1;
        }
        // default (-1): past 20 iterations when the follow-up works in LDS AND the batch is at most three times what the device holds at once
        // (re-measured in round 6 under the default QP solver profile, whose solves are shorter - profiles/r06_handover_co.txt: with the
        // follow-up kernel beside the launch -18 % per tick at 4 096 instances, -13 % at 8 192, -4 % at 16 384, 0 at 32 768, +1 % at
        // 65 536; with it only behind the launch nothing is gained any more at any size), never when it would run over the planes in HBM (a
        // loss: profiles/r05_handover.txt)
        const bool small = c.qp > 0 && B <= 3 * c.qp;
        p.hand_iter = in.handover_iter > 0 ? in.handover_iter : ((c.resume_lds && small) ? 20 : 0);
        p.hand_ready = c.resume > 0;
        p.hand = p.hand_ready && p.hand_iter > 0;
        p.hand_lds = c.resume_lds;
        p.hand_bytes = c.resume_lds ? lbytes : xbytes;
        p.hand_wgs = std::min(c.resume, B);
    }
    if (!p.hand) p.hand_iter = 0;
    // The follow-up kernel BESIDE the draining launch (usv_qp_resume_co): on a stream of its own, eligible together with the main launch;
    // what it does not get to is done by the follow-up launch behind the main one.  With the planes copied into LDS only (the form that pays).
    p.co = p.hand && in.handover_co != 0 && c.resume_lds && in.has_resume_co && in.own_stream;
    // One follow-up workgroup per CU unless the caller asks otherwise (option "handover_co_wgs"): what finds room BESIDE the main launch's
    // workgroups at once (75 KB of LDS next to their eight times 10 KB).  With two per CU - what fits once the main launch has left - some
    // of them wait to be placed while the main launch runs, and about one tick in 1 500 then stalled until their waits ran out: the main
    // launch took 410 ms instead of 9 (tools/co_soak.py, docs/rounds/r06.md section 8: 0 stalls in 16 000 ticks with one per CU, same pace).
    if (p.co) p.co_wgs = std::min(p.hand_wgs, in.co_wgs > 0 ? in.co_wgs : std::max(ncu, 1L));
    return p;
}

} // namespace usv
