// usvmpc.hip — gfx950 kernels + the C ABI of include/usvmpc.h.
//
// Two kernels per SQP-RTI iteration (and per iteration of the full SQP):
//   usv_linearize<M,KCH,..>   one 16-lane group per (instance, stage): ERK4 + forward VDE, GN gradient, the
//                             stage matrix packed into the workspace planes   (linearize.hpp)
//   usv_qp_rti<M,KCH,SOFT,..> one 16-lane group per instance: obstacle-row linearisation, Riccati-IPM QP,
//                             RTI / SQP step, NLP residual test for the full SQP  (qp_ipm.hpp)
// Both are FP64 VALU + DPP kernels (lane gathers go through the LDS crossbar, no LDS memory, no MFMA: the
// blocks are at most 16x16).
//
// Build parts.  The QP kernel templates are what takes minutes to compile, and one (model, obstacle chunks) pair has nothing in common
// with another: __graft_entry__.build() therefore compiles THIS file several times in parallel, -DUSV_PART=0 for the C ABI, the handle
// bookkeeping, the launches (launch_qp carries out the plan of qp_plan.hpp, where the launch policy lives as a host-only function of plain
// numbers: tests/test_qp_plan.py; launch_solve likewise the plan of lin_plan.hpp - the lineariser's schedule, maps and grids:
// tests/test_lin_plan.py; copy_field the field table and the host mirror's bookkeeping of field_plan.hpp: tests/test_field_plan.py;
// usvmpc_set_option the option table of option_plan.hpp: tests/test_option_plan.py; carry_world the front ends' world list of
// world_plan.hpp: tests/test_world_plan.py)
// and the small kernels, -DUSV_PART=1 .. 5 for the kernels of one pair each - the kernel table
// kernels_for<M, KCH, SOFT> (explicit instantiation in its part, extern template in part 0, which calls it) - and links the objects.
// Without USV_PART everything is one translation unit (the generated-model libraries of genbuild.py).
#ifndef USV_PART
#define USV_PART -1
#endif
#define USV_MAIN (USV_PART <= 0)

#include "gfx950/lanes.hpp"

#include "ca_fleet_world.hpp"
#include "cascade.hpp"
#include "cascade_log_plan.hpp"
#include "closed_loop_log.hpp"
#include "cost_eval.hpp"
#include "fleet_world.hpp"
#include "guidance.hpp"
#include "host_spec.hpp"
#include "lanes_probe.hpp"
#include "lin_plan.hpp"
#include "log_plan.hpp"
#include "linearize.hpp"
#include "models.hpp"
#include "obstacle_tracks.hpp"
#include "option_plan.hpp"
#include "pf_guidance.hpp"
#include "qp_ipm.hpp"
#include "qp_plan.hpp"
#include "sim.hpp"
#include "world_plan.hpp"
#include "cond_launch.hpp"
#include "field_plan.hpp"
#include "fleet_plan.hpp"
#ifdef USV_GEN_MODEL_HEADER // a model generated from a symbolic definition (codegen.py): struct ModelGen
#include USV_GEN_MODEL_HEADER
#endif

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

using namespace usv;

// ---------------------------------------------------------------------------------- kernels
#ifndef USV_LIN_BLOCKS
#define USV_LIN_BLOCKS 2 // 256-thread blocks per CU the lineariser is compiled for (2: 2 waves per SIMD, 256 registers)
#endif
// MODE: 0 the whole batch; 1 / 3 speculative for the next tick beside a running QP launch; 2 / 4 fix-up of what that pass skipped (linearize.hpp)
// Workgroups and what `n` counts:
//   0, 1, 2  256 threads, 16 (group, stage) pairs in stage-major order, n pairs
//   3        ONE wave, 4 work items of lin_order.hpp, n items.  The QP launch it runs beside holds every SIMD's registers (2 waves x 256); a QP
//            wave that leaves frees room for one of these waves (224 registers), on that SIMD only - a four-wave workgroup has to wait
//            until each of the CU's SIMDs has lost a QP wave.
//   4        256 threads = 4 waves, one wave per group (its rows share out the group's marked stages), n groups
// PAIR (models with PairCols, params.hpp; option "lin_pairs"): a 16-lane row serves two (group, stage) pairs (Linearize::run_pair_at), the workgroups
// are the same and n counts ROWS for MODE 0 - 3: 0, 1, 2 the pairs in the same stage-major order, two to a row; 3 the rows of the retire
// order, padded to whole waves (lin_order.hpp: a wave takes 8 items, the two of a row from one instance); 4 groups as before, the marked
// stages shared out over the wave's eight halves.
// (LIN_MODES, lin_block and the grids: lin_plan.hpp)
template <class M, int KCH, bool SOFT, bool MULTI, bool PAIR = false, int MODE = 0>
__global__ void __launch_bounds__(lin_block(MODE), USV_LIN_BLOCKS) usv_linearize(DevPtrs P, long n)
{
    using L = Linearize<M, KCH, SOFT, MULTI, MODE>;
    if constexpr (MODE == 4) {
        const long g = (long)blockIdx.x * (lin_block(MODE) / 64) + (long)(threadIdx.x >> 6);
        if constexpr (PAIR) { if (g < n) L::run_pair_marked(P, g, (int)lanes::wave_row()); }
        else if (g < n) L::run_marked(P, g, (int)lanes::wave_row());
    } else if constexpr (PAIR) {
        const long row = lanes::group_linear();
        if (row >= n) return; // (n is a multiple of 4, lin_order.hpp: whole waves leave together)
        if constexpr (MODE == 3) L::run_pair_item(P, row);
        else L::run_pair(P, row);
    } else {
        const long gid = lanes::group_linear();
        if (gid >= n) return; // n is a multiple of 4: whole waves leave together
        if constexpr (MODE == 3) L::run_item(P, gid);
        else L::run(P, gid);
    }
}

#ifndef USV_QP_WAVES
#define USV_QP_WAVES 2 // waves per SIMD the QP kernel is compiled for (register budget 512 / USV_QP_WAVES)
#endif
// Two obstacle chunks (K > 16) or soft state bounds keep twice the row state in flight: those instantiations get the whole
// register file of a SIMD (one wave, 512 registers) instead of spilling 100-280 registers at two waves - the kernel is
// issue-bound, a second wave buys little and scratch traffic costs a lot.
template <int KCH, bool SOFTBOX>
constexpr int qp_waves() { return (KCH >= 2 || SOFTBOX) ? 1 : USV_QP_WAVES; }

// rows: instances a wave starts on (4; fewer when the workspace lives in LDS and only that many fit: LDSWS) - row r of block b
// starts on group b * rows + r, surplus rows stay idle.
// AUXLDS: the aux plane of the rows' instances in the wave's LDS instead of HBM (qp_ipm.hpp)
// WIDE: the latency mapping - one instance per wave (rows = 1: rows 1 - 3 are handed row 0's group and share its LDS region; in the
// sweeps they take over the row work of the neighbouring stages: qp_ipm.hpp)
// WW > 1 (with WIDE): a workgroup of WW waves per instance (qp_ipm.hpp)
// CPC: with HPIPM's conditional predictor-corrector built in (qp_ipm.hpp; option "cond_pred_corr" switches the test) - every kernel of the library
template <class M, int KCH, bool SOFT, bool HDIAG, bool PACK, bool SOFTBOX, bool LDSWS = false, bool MERGE = false, bool AUXLDS = false, bool WIDE = false,
          int WW = 1, bool CPC = true>
__global__ void __launch_bounds__(64 * WW, ((LDSWS || WIDE) ? 1 : qp_waves<KCH, SOFTBOX>())) usv_qp_rti(DevPtrs P, long ngroups, int phase, int queue0, int rows)
{
    const int row = (int)(threadIdx.x >> 4);
    const long g0 = (long)blockIdx.x * rows;
    if (g0 >= ngroups) return;
    // (hand-over with a co-resident follow-up kernel: that kernel goes to work only once every workgroup of THIS launch is on the device)
    if constexpr (!WIDE && !LDSWS) { if (P.co_ctl != nullptr && threadIdx.x == 0) lanes::count_one(P.co_ctl + 2); }
    const bool has = row < rows;
    QpIpm<M, KCH, SOFT, HDIAG, PACK, SOFTBOX, LDSWS, MERGE, AUXLDS, WIDE, WW, CPC> q(P, has ? g0 + row : g0, has ? row : -1);
    q.solve(phase, queue0);
}
// The wide instantiations: packed layouts with one or two obstacle chunks, and the layouts with the box rows in planes of their own (UNPACKED:
// no obstacle rows, obstacle rows that leave the box rows no idle lanes, or - SOFTBOX - soft state bounds).
// (LDSWS: the solver's planes in LDS - false: in HBM, for horizons that do not fit a CU's LDS and for the launches of a full SQP)
template <class M, int KCH, bool SOFT, bool MERGE, bool LDSWS = true, int WW = 1, bool SOFTBOX = false, bool UNPACKED = false>
constexpr auto wide_kernel()
{
    // (unpacked rows beside obstacle rows and soft state bounds: one wave per instance; four waves are built for the packed layouts - one or two
    // obstacle chunks, K = 17 .. 32 being BASELINE configs[4]'s OCP - and the layout without obstacle rows)
    if constexpr (SOFTBOX || (UNPACKED && KCH > 0)) {
        if constexpr (WW == 1 && !MERGE) return &usv_qp_rti<M, KCH, SOFT, true, false, SOFTBOX, LDSWS, false, false, true, 1>;
        else return (decltype(&usv_qp_rti<M, KCH, SOFT, true, false, SOFTBOX, true, false>))nullptr;
    } else if constexpr (KCH == 1 || KCH == 2) return &usv_qp_rti<M, KCH, SOFT, true, true, false, LDSWS, MERGE, false, true, WW>;
    else if constexpr (KCH == 0 && !MERGE) return &usv_qp_rti<M, KCH, SOFT, true, false, false, LDSWS, false, false, true, WW>; // (no obstacle rows: box rows in their own planes)
    else return (decltype(&usv_qp_rti<M, KCH, SOFT, true, (KCH > 0), false, true, MERGE>))nullptr;
}
// The follow-up of a launch that handed long runners over (QpIpm::suspend, option "handover_iter"): one wave per suspended instance,
// on the latency mapping - over the planes in HBM the suspending row was working on, or (LDSWS, horizons that fit) after copying them into
// LDS, where a pass costs half.  Workgroup i takes entries i, i + gridDim, ... of the list; with an empty list the launch is a few microseconds.
template <class M, int KCH, bool SOFT, bool MERGE, bool LDSWS>
__global__ void __launch_bounds__(64, 1) usv_qp_resume(DevPtrs P)
{
    const int n = lanes::uniform(*P.susp_count);
    const bool co = P.co_ctl != nullptr; // (the co-resident kernel may have taken the entry - or be about to: one compare-and-swap decides)
    for (int i = (int)blockIdx.x; i < n; i += (int)gridDim.x) {
        int g = P.susp_list[i];
        if (co) {
            if (threadIdx.x == 0) g = (g >= 0 && lanes::claim(P.susp_list + i, g)) ? g : -1;
            g = lanes::wave_first_i(g);
            if (g < 0) continue;
        }
        QpIpm<M, KCH, SOFT, true, (KCH > 0), false, LDSWS, MERGE, false, true, 1> q(P, (long)g, (threadIdx.x >> 4) == 0 ? 0 : -1);
        q.solve(3, -1);
    }
}
// The same follow-up BESIDE the draining launch (option "handover_co"): enqueued on a stream of its own together with the main launch, its
// workgroups come onto the device as main wavefronts leave it (75 KB of LDS and a SIMD's registers each), take a ticket each and wait - a
// bounded wait - for the list entry of that number to appear; the instance behind it is finished here while the main launch is still
// draining, instead of behind it.  A workgroup leaves when the main launch has ended and its ticket's entry never came (the list is
// complete then), when its wait runs into the spin limit, or - at once - when it finds itself on the device before every workgroup of the
// main launch is (it must not hold what a persistent launch still waits for).  Whatever is left is done by usv_qp_resume behind the main
// launch; an entry is taken by one of the two (compare-and-swap).  Scheduling only: the same sweeps over the same planes.
template <class M, int KCH, bool SOFT, bool MERGE>
__global__ void __launch_bounds__(64, 1) usv_qp_resume_co(DevPtrs P, int main_wgs, int cap, int spin_limit)
{
    int *ctl = P.co_ctl;
    {
        int ok = 0;
        if (threadIdx.x == 0) ok = lanes::observe(ctl + 2) >= main_wgs;
        if (!lanes::wave_first_i(ok)) return;
    }
    for (;;) {
        int t = 0;
        if (threadIdx.x == 0) t = atomicAdd(ctl, 1);
        t = lanes::wave_first_i(t);
        if (t >= cap) return;
        // Every lane polls the same word: one access for the wave, and NO loop inside a single-lane region.  (The first form of this kernel had
        // lane 0 alone run the ticket / poll / claim loops: on this toolchain every instance a workgroup finished after its first came out
        // wrong - with or without the main launch beside it, with or without the fences; the sweeps' code was the follow-up launch's.  The
        // single-lane regions left are an atomic each.)
        int e, spins = 0;
        for (;;) {
            e = lanes::observe(P.susp_list + t);
            if (e != -1) break;
            if (lanes::observe(ctl + 1) != 0) { e = lanes::observe(P.susp_list + t); break; } // (the main launch has ended: the list is final)
            if (++spins > spin_limit) break;
            __builtin_amdgcn_s_sleep(64);
        }
        e = lanes::wave_first_i(e);
        if (e == -1) { // nothing will come for this number (entries are dense), or the wait was given up: what is left is the launch's behind the main one
            if (spins > spin_limit && threadIdx.x == 0) lanes::count_one(ctl + 4);
            return;
        }
        int mine = 0;
        if (threadIdx.x == 0) mine = (e >= 0 && lanes::claim(P.susp_list + t, e)) ? 1 : 0;
        if (!lanes::wave_first_i(mine)) continue;
        lanes::acquire_agent(); // (the suspending wave released at agent scope before the entry went out)
        {
            QpIpm<M, KCH, SOFT, true, (KCH > 0), false, true, MERGE, false, true, 1> q(P, (long)e, (threadIdx.x >> 4) == 0 ? 0 : -1);
            q.solve(3, -1);
        }
        if (threadIdx.x == 0) lanes::count_one(ctl + 3);
    }
}
static __global__ void usv_co_done(int *ctl) { lanes::publish(ctl + 1, 1); }
using qp_resume_t = void (*)(DevPtrs);
using qp_resume_co_t = void (*)(DevPtrs, int, int, int);
template <class M, int KCH, bool SOFT, bool MERGE, bool LDSWS = false>
constexpr qp_resume_t resume_kernel()
{
    if constexpr (KCH == 1 || (KCH == 0 && !MERGE)) return &usv_qp_resume<M, KCH, SOFT, MERGE, LDSWS>;
    else return nullptr;
}
template <class M, int KCH, bool SOFT, bool MERGE>
constexpr qp_resume_co_t resume_co_kernel()
{
    if constexpr (KCH == 1 || (KCH == 0 && !MERGE)) return &usv_qp_resume_co<M, KCH, SOFT, MERGE>;
    else return nullptr;
}
using qp_kernel_t = void (*)(DevPtrs, long, int, int, int);
using group_kernel_t = void (*)(DevPtrs, long); // (the lineariser, the multiplier read-back)

// The kernels of one (model, obstacle chunks) pair for the handle's current row layout (kernels_for), and what the launch policy needs to
// know about them.  A null kernel: that mapping does not exist for the layout.
struct Kernels {
    qp_kernel_t qp[SLOT_QP_KERNELS];             // by QpSlot (qp_plan.hpp): four instances per wave, the latency mapping
    qp_resume_t resume, resume_lds;              // the follow-up launch of a hand-over: over the planes in HBM / after copying them into LDS
    qp_resume_co_t resume_co;                    // ... and its co-resident form (usv_qp_resume_co)
    int nplw, ex_lds, ex_hbm;                    // planes per stage an instance keeps in LDS; planes of the exchange area (qp_ipm.hpp NPLW, EX_N)
    group_kernel_t lin[2][LIN_MODES];            // usv_linearize [MULTI][MODE]
    group_kernel_t lin_pair[2][LIN_MODES];       // ... two pairs per row (PAIR); null: the model does not declare its columns (PairCols)
    group_kernel_t qp_export;                    // usv_qp_export
    int npt_hard, npt_soft;                      // WsLayout::NPT without / with soft state bounds
    int kch;                                     // the instantiation's KCH and SOFT (h->kch / h->soft may differ: usv_model with "soft" set)
    bool soft;
};

template <class M, int KCH, bool SOFT, bool MERGE, bool SOFTBOX = false, bool UNPACKED = false>
void set_wide(Kernels &k)
{
    using WL = WsLayout<M, KCH, SOFT, SOFTBOX>;
    constexpr bool packed = KCH > 0 && !SOFTBOX && !UNPACKED; // (the packed layouts leave the four box planes out of the LDS map)
    constexpr bool resumes = !(SOFTBOX || (UNPACKED && KCH > 0));
    k.qp[SLOT_WIDE_LDS1] = wide_kernel<M, KCH, SOFT, MERGE, true, 1, SOFTBOX, UNPACKED>();
    k.qp[SLOT_WIDE_HBM1] = wide_kernel<M, KCH, SOFT, MERGE, false, 1, SOFTBOX, UNPACKED>();
    k.qp[SLOT_WIDE_LDS4] = wide_kernel<M, KCH, SOFT, MERGE, true, 4, SOFTBOX, UNPACKED>();
    k.qp[SLOT_WIDE_HBM4] = wide_kernel<M, KCH, SOFT, MERGE, false, 4, SOFTBOX, UNPACKED>();
    k.resume = resumes ? resume_kernel<M, KCH, SOFT, MERGE>() : nullptr;
    k.resume_lds = resumes ? resume_kernel<M, KCH, SOFT, MERGE, true>() : nullptr;
    k.resume_co = resumes ? resume_co_kernel<M, KCH, SOFT, MERGE>() : nullptr;
    k.nplw = WL::P_RB0 - (packed ? 4 : 0) + (SOFTBOX ? 6 : 0);
    k.ex_lds = wide_ex_planes(KCH, SOFTBOX);
    k.ex_hbm = wide_ex_planes_hbm(KCH, SOFTBOX);
}

// Multiplier read-back (usvmpc_get "lam" / "t"): the inequality multipliers and slacks of every instance's last QP, from the
// group-indexed workspace planes into instance-major arrays in acados' row order (QpIpm::export_rows).  Run on demand.
template <class M, int KCH, bool SOFT, bool PACK, bool SOFTBOX>
__global__ void __launch_bounds__(64) usv_qp_export(DevPtrs P, long ngroups)
{
    const long g0 = (long)blockIdx.x * 4;
    if (g0 >= ngroups) return;
    QpIpm<M, KCH, SOFT, true, PACK, SOFTBOX> q(P, g0 + (long)(threadIdx.x >> 4));
    q.export_rows();
}

// Instances of a launch whose QP did not converge to the IPM tolerances (qp_status != 0): counted by a kernel of its own behind the QP
// launch, per workgroup in LDS and one atomic per workgroup (usvmpc_unconverged_counts; SURVEY.md 8(d) counts converged solves).  Not inside
// QpIpm::finish(): one more counter there moved the headline kernel's register allocation (12 -> 17 spilled registers, +1.3 % per launch in a
// same-box A/B).
static __global__ void __launch_bounds__(256) usv_count_unconverged(const int *qp_status, int B, int *count, unsigned long long *total)
{
    __shared__ int loc;
    if (threadIdx.x == 0) loc = 0;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B && qp_status[i] != 0) atomicAdd(&loc, 1);
    __syncthreads();
    if (threadIdx.x == 0 && loc != 0) { atomicAdd(count, loc); atomicAdd(total, (unsigned long long)loc); } // (total: the handle's running sum)
}

#if USV_MAIN
// full SQP bookkeeping: start of a call (everything running) and end (still running = max iterations)
__global__ void usv_sqp_begin(DevPtrs P, int B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) { P.sqp_state[i] = -1; P.sqp_iter[i] = 0; }
}
__global__ void usv_sqp_end(DevPtrs P, int B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) P.status[i] = P.sqp_state[i] < 0 ? 2 : P.sqp_state[i];
}

// Closed-loop hand-over between two ticks, as the reference's callers do it on the host
// (x0 = get(1,"x"); set(0,"lbx",x0): scripts/usv_guidance_ca1/main.py:169-175): the next initial
// state is the predicted x_1 plus an optional Gaussian disturbance (the commented "Add noise"
// hooks of scripts/usv_pf_ca/main.py:181-183).  No trajectory shift, as in the reference.
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// sigma * N(0,1) for state j of instance g: key = g * nx + j, g the instance's GLOBAL index (option "instance_offset" + its index in the
// handle), so that a batch split over several handles draws the same disturbances as one handle over the whole batch (Box-Muller)
__device__ __forceinline__ double noise(double sigma, unsigned long long seed, unsigned long long key)
{
    const unsigned long long h1 = splitmix64(seed ^ (2 * key));
    const unsigned long long h2 = splitmix64(seed ^ (2 * key + 1));
    const double u1 = ((double)(h1 >> 11) + 1.0) * (1.0 / 9007199254740993.0);
    const double u2 = (double)(h2 >> 11) * (1.0 / 9007199254740992.0);
    return sigma * sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

__global__ void usv_advance(DevPtrs P, int nx, double sigma, unsigned long long seed, unsigned mask, long long offset)
{
    const DevSpec &S = *P.spec;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)S.B * nx) return;
    const long b = i / nx;
    const int j = (int)(i - b * nx);
    double v = P.x[(b * (S.N + 1) + 1) * nx + j];
    if (sigma != 0.0 && ((mask >> j) & 1u)) v += noise(sigma, seed, (unsigned long long)((offset + b) * nx + j));
    const_cast<double *>(P.x0)[i] = v;
}

// The plant step of a closed loop with a plant of its own (usvmpc_advance_sim): x0 <- sim(x0, u_0) over T in `steps` RK4 steps (sim.hpp,
// one lane per instance), plus the disturbance of usv_advance.  In place: a thread reads its instance's x0 whole before it writes it.
template <class M>
__global__ void __launch_bounds__(256) usv_advance_sim(DevPtrs P, double T, int steps, double sigma, unsigned long long seed, unsigned mask,
                                                       long long offset)
{
    constexpr int NX = M::NX, NU = M::NU;
    const DevSpec &S = *P.spec;
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (long)S.B) return;
    double *x0 = const_cast<double *>(P.x0) + b * NX;
    const double *u0 = P.u + b * (long)S.N * NU;
    double x[NX], U[NU > 0 ? NU : 1], s[NX], su[NU > 0 ? NU : 1];
    sfor<0, NX>([&](auto i) { x[i] = x0[i]; s[i] = 0.0; });
    sfor<0, NU>([&](auto l) { U[l] = u0[l]; su[l] = 0.0; });
    erk_period<M, false>(x, U, s, su, T, steps);
    sfor<0, NX>([&](auto j) {
        double v = x[j];
        if (sigma != 0.0 && ((mask >> j) & 1u)) v += noise(sigma, seed, (unsigned long long)((offset + b) * NX + j));
        x0[j] = v;
    });
}

// ---- Closed-loop log (usvmpc_log_*; the schedule and layout: log_plan.hpp; the arithmetic: closed_loop_log.hpp).
// usv_log_record: one launch per hand-over that records or accumulates, enqueued AHEAD of the hand-over's own kernel, so that x0 is still the
// state the solve saw.  It reads x0, u, status and qp_iter and writes log memory only.  Thread t serves element t of each of the record's
// three slabs and of the sums (four guards): every store of a wave is one contiguous run (512 B of doubles), the reads gather inside an
// instance's x0 row.  The selected states and the error channels' states travel as nibble lists in two 64-bit arguments, the constants as
// four scalars picked by a select chain - nothing in the argument struct is indexed at run time.
__global__ void __launch_bounds__(256) usv_log_record(LogRec R)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (R.rx && t < R.B * R.nsel) {
        const long b = t / R.nsel;
        const int j = (int)(t - b * R.nsel);
        R.rx[t] = R.x0[b * R.nx + log_nibble(R.sel, j)];
    }
    if (R.ru && t < R.B * R.nu) {
        const long b = t / R.nu;
        const int l = (int)(t - b * R.nu);
        R.ru[t] = R.u[b * R.ustride + l];
    }
    if (R.rs && t < R.B) R.rs[t] = R.status[t] | (R.qp_iter[t] << 8);
    if (R.sum_abs && t < R.B * R.n_err) {
        const long b = t / R.n_err;
        const int c = (int)(t - b * R.n_err);
        const double *x = R.x0 + b * R.nx;
        const double k = c == 0 ? R.c0 : c == 1 ? R.c1 : c == 2 ? R.c2 : R.c3;
        const double rhs = ((R.err_const >> c) & 1u) ? k : x[log_nibble(R.err_b, c)];
        double sa = R.sum_abs[t], sq = R.sum_sq[t];
        log_accumulate(log_error(x[log_nibble(R.err_a, c)], rhs), &sa, &sq);
        R.sum_abs[t] = sa;
        R.sum_sq[t] = sq;
    }
}

// ---- Objective value (usvmpc_get "cost" / "cost_stage" / "cost_parts", usvmpc_eval_cost, usvmpc_cost_track; the arithmetic and the order of
// every sum: cost_eval.hpp).  Both kernels read arrays a caller can get (x, u, yref, yref_e, sl, su, x0) and write cost memory only.
// One 16-lane group per (instance, stage): lane r owns row r of V and of W (16 + 16 registers, from the transposed device table CostTab: a
// kernel argument indexed at run time would be scratch - usv_log_record's trap) and loads element r of the stage's z and yref row, so a
// group's loads are contiguous runs; z_j, r_j and the rows' shares of q reach the other lanes through lanes::bcast<j> in unrolled loops whose
// bounds are compile-time constants - sequential sums, no butterfly.
struct CostRows {
    double V[COST_LANES], W[COST_LANES];
};
__device__ __forceinline__ void cost_load_rows(CostRows &R, const double *Vt, const double *Wt, int lane)
{
    sfor<0, COST_LANES>([&](auto j) { R.V[j] = Vt[j * COST_LANES + lane]; R.W[j] = Wt[j * COST_LANES + lane]; });
}
// q of the group's stage, in every lane: z and yr are this lane's entries, 0.0 beyond nz / ny.  Every loop runs to 16 over the zero-padded
// tables without a guard (16 + 16 + 16 + 32 hoisted lane masks cost the kernel a hundred scalar registers): a padded term is 0.0 * 0.0, and
// adding +0.0 to a sum that started from +0.0 leaves its bits as they are (such a sum is never -0.0) - cost_eval.hpp, "padding".
__device__ __forceinline__ double cost_group_q(const CostRows &R, double z, double yr)
{
    double y = 0.0;
    sfor<0, COST_LANES>([&](auto j) { y = cost_mac(y, R.V[j], lanes::bcast<j>(z)); });
    const double r = cost_sub(y, yr);
    double t = 0.0;
    sfor<0, COST_LANES>([&](auto j) { t = cost_mac(t, R.W[j], lanes::bcast<j>(r)); });
    const double p = cost_mul(r, t);
    double q = 0.0;
    sfor<0, COST_LANES>([&](auto i) { q = cost_add(q, lanes::bcast<i>(p)); });
    return q;
}
// S of the group's stage, in every lane: t0 / t1 are this lane's cost_slack_term of rows lane / 16 + lane (0.0 beyond Ks)
__device__ __forceinline__ double cost_group_S(double t0, double t1, int Ks)
{
    double S = 0.0;
    sfor<0, COST_LANES>([&](auto i) { S = cost_add(S, lanes::bcast<i>(t0)); });
    if (Ks > COST_LANES) sfor<0, COST_LANES>([&](auto i) { S = cost_add(S, lanes::bcast<i>(t1)); });
    return S;
}
// what lane `lane` of a group loads for stage k < N of instance b: its entry of z = [u_k; xs] and of yref, its slack terms (xs: x_k, or x0).
// SOFT false (hard h rows, or none): no slack term exists - neither loads nor registers for them.
template <bool SOFT> struct CostIn;
template <> struct CostIn<false> {
    double z, yr;
};
template <> struct CostIn<true> {
    double z, yr, sl0, su0, sl1, su1;
};
template <bool SOFT>
__device__ __forceinline__ CostIn<SOFT> cost_load_stage(const CostArgs &A, const double *xs, long b, int k, int lane)
{
    CostIn<SOFT> I;
    const long bk = b * A.N + k;
    const int nz = A.nu + A.nx;
    const double *pz = lane < A.nu ? A.u + bk * A.nu + lane : xs + (lane - A.nu);
    I.z = lane < nz ? *pz : 0.0;
    I.yr = lane < A.ny ? A.yref[bk * A.ny + lane] : 0.0;
    if constexpr (SOFT) {
        const double *sl = A.sl + bk * A.K, *su = A.su + bk * A.K;
        I.sl0 = lane < A.Ks ? sl[lane] : 0.0;
        I.su0 = lane < A.Ks ? su[lane] : 0.0;
        I.sl1 = COST_LANES + lane < A.Ks ? sl[COST_LANES + lane] : 0.0;
        I.su1 = COST_LANES + lane < A.Ks ? su[COST_LANES + lane] : 0.0;
    }
    return I;
}
// this lane's penalties of rows lane and 16 + lane (zero beyond Ks: the table is zero-padded)
template <bool SOFT> struct CostPen;
template <> struct CostPen<false> {};
template <> struct CostPen<true> {
    double zl0, zu0, Zl0, Zu0, zl1, zu1, Zl1, Zu1;
};
template <bool SOFT>
__device__ __forceinline__ CostPen<SOFT> cost_load_pen(const CostTab *T, int lane)
{
    if constexpr (SOFT)
        return CostPen<true>{T->zl[lane], T->zu[lane], T->Zl[lane], T->Zu[lane], T->zl[16 + lane], T->zu[16 + lane], T->Zl[16 + lane], T->Zu[16 + lane]};
    else
        return CostPen<false>{};
}
// ls_k and slack_k of the group's stage, in every lane (hard rows: slack_k = dt * 0.0)
template <bool SOFT>
__device__ __forceinline__ void cost_group_stage(const CostArgs &A, const CostRows &R, const CostPen<SOFT> &P, const CostIn<SOFT> &I, double &ls, double &slack)
{
    ls = cost_ls(A.dt, cost_group_q(R, I.z, I.yr));
    double S = 0.0;
    if constexpr (SOFT) {
        const double t0 = cost_slack_term(P.zl0, P.zu0, P.Zl0, P.Zu0, I.sl0, I.su0);
        const double t1 = cost_slack_term(P.zl1, P.zu1, P.Zl1, P.Zu1, I.sl1, I.su1);
        S = cost_group_S(t0, t1, A.Ks);
    }
    slack = cost_mul(A.dt, S);
}
// the value lane `src` of the wave holds, as a wave-uniform number
__device__ __forceinline__ double cost_from_lane(double v, int src)
{
    const long l = __builtin_bit_cast(long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(l & 0xffffffffL), src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(l >> 32), src);
    return __builtin_bit_cast(double, (long)(((unsigned long)hi << 32) | lo));
}

// usv_cost_eval: ONE wave per instance (four to a workgroup).  The wave's four groups take four consecutive stages k < N at a time (a PASS) -
// their loads of x, u, yref, sl and su join up into one contiguous run each.  The arithmetic of a pass is some 150 FP64 instructions in a
// dependent chain, so what keeps HBM busy is how many passes' loads a wave has in flight: COST_AHEAD passes are loaded ahead of the one
// being worked on, in a ring whose slots are compile-time indices (two doubles per lane and pass for hard rows, six for soft ones).  The
// stages' values then enter the instance's three running sums one by one in stage order (wave-uniform numbers read from lanes 0, 16, 32,
// 48), so the totals need neither a second pass nor a per-stage buffer for the two shares.  A group past stage N - 1 works on stage N - 1
// again and neither stores nor enters the sums (control flow stays wave-uniform around the DPP reads).  Stage N comes last, on the terminal
// tables, which take over the stage tables' registers.
constexpr int COST_AHEAD = 4;
template <bool SOFT>
__global__ void __launch_bounds__(256) usv_cost_eval(CostArgs A)
{
    const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= A.B) return; // (a whole wave)
    const int lane = lanes::lane(), row = (int)lanes::wave_row();
    const CostPen<SOFT> P = cost_load_pen<SOFT>(A.tab, lane);
    CostRows R;
    cost_load_rows(R, A.tab->Vt, A.tab->Wt, lane);
    const double *xb = A.x + b * (long)(A.N + 1) * A.nx;
    double total = 0.0, p_ls = 0.0, p_slack = 0.0;
    const int last = A.N - 1;
    auto load = [&](int k0) { // (the pass that starts at stage k0; past the end: stage N - 1 again)
        const int k = k0 + row < last ? k0 + row : last;
        return cost_load_stage<SOFT>(A, xb + (long)k * A.nx, b, k, lane);
    };
    CostIn<SOFT> ring[COST_AHEAD];
    sfor<0, COST_AHEAD>([&](auto d) { ring[d] = load(4 * d); });
    for (int k0 = 0; k0 < A.N; k0 += 4 * COST_AHEAD) {
        sfor<0, COST_AHEAD>([&](auto d) {
            const int kd = k0 + 4 * d;
            if (kd < A.N) { // (wave-uniform)
                const CostIn<SOFT> I = ring[d];
                ring[d] = load(kd + 4 * COST_AHEAD);
                double ls, slack;
                cost_group_stage<SOFT>(A, R, P, I, ls, slack);
                const double c = cost_add(ls, slack);
                if (kd + row < A.N && lane == 0) A.cost_stage[b * (A.N + 1) + kd + row] = c;
                sfor<0, 4>([&](auto g) {
                    if (kd + g < A.N) {
                        total = cost_add(total, cost_from_lane(c, 16 * g));
                        if constexpr (SOFT) {
                            p_ls = cost_add(p_ls, cost_from_lane(ls, 16 * g));
                            p_slack = cost_add(p_slack, cost_from_lane(slack, 16 * g));
                        }
                    }
                });
            }
        });
    }
    // (hard rows: slack_k = dt * 0.0 = +0.0 and c_k = ls_k + 0.0 = ls_k to the bit - ls_k is never -0.0 - so the sum of the ls_k is the
    // sum of the c_k, the same additions in the same order, and the sum of the slack_k stays +0.0)
    if constexpr (!SOFT) p_ls = total;
    cost_load_rows(R, A.tab->Vte, A.tab->Wte, lane);
    const double zN = lane < A.nx ? xb[(long)A.N * A.nx + lane] : 0.0;
    const double yN = lane < A.ny_e ? A.yref_e[b * A.ny_e + lane] : 0.0;
    const double cN = cost_mul(0.5, cost_group_q(R, zN, yN));
    total = cost_add(total, cN);
    if (threadIdx.x % 64 == 0) {
        A.cost_stage[b * (A.N + 1) + A.N] = cN;
        A.cost[b] = total;
        A.parts[b * 3 + 0] = p_ls;
        A.parts[b * 3 + 1] = cN;
        A.parts[b * 3 + 2] = p_slack;
    }
}

// usv_cost_track: sum[b] += c_0(x0[b], u[b][0], yref[b][0], sl[b][0], su[b][0]), a 16-lane group per instance (the same rows-over-lanes
// arithmetic: every lane's load is its element of a contiguous run, none walks a row of its own), enqueued by a hand-over AHEAD of its own
// kernel so that x0 is still the state the solve saw.  A group serves up to COST_TRACK_EACH instances, G groups apart, so that its 32
// table loads are paid once, with the next instance's loads issued ahead of the current one's arithmetic.  A group past the batch works on
// the last instance again and stores nothing.
constexpr int COST_TRACK_EACH = 4;
template <bool SOFT>
__global__ void __launch_bounds__(256) usv_cost_track(CostArgs A)
{
    const long g = lanes::group_linear(), G = (long)gridDim.x * (blockDim.x >> 4);
    const int lane = lanes::lane();
    const CostPen<SOFT> P = cost_load_pen<SOFT>(A.tab, lane);
    CostRows R;
    cost_load_rows(R, A.tab->Vt, A.tab->Wt, lane);
    auto load = [&](long b) {
        b = b < A.B ? b : A.B - 1;
        return cost_load_stage<SOFT>(A, A.x0 + b * A.nx, b, 0, lane);
    };
    CostIn<SOFT> In = load(g);
    sfor<0, COST_TRACK_EACH>([&](auto it) {
        const long b = g + it * G;
        const CostIn<SOFT> I = In;
        if (it + 1 < COST_TRACK_EACH) In = load(b + G);
        double ls, slack;
        cost_group_stage<SOFT>(A, R, P, I, ls, slack);
        const double c = cost_add(ls, slack);
        if (b < A.B && lane == 0) A.sum[b] = cost_add(A.sum[b], c);
    });
}

// ---- Obstacle tracks (option "obstacle_tracks"; the arithmetic: obstacle_tracks.hpp).
// usv_obstacle_predict: p of every stage from the tracks, p[b][k][slot] = pos[b][slot] + (k dt) vel[b][slot] - a pure streaming write (1.7 GB at
// N = 80, K = 20, 65 536 instances), one 16-byte store per (ox, oy) pair.  One workgroup per instance: thread t owns slot t % K of stage
// offset t / K (divided once), keeps its pair of the tracks in registers and walks the stages in steps of 256 / K, so that in every pass the live
// lanes write 256 / K whole stages = ONE contiguous run of p, lane t the t-th pair of it (a wave's stores cover 1 KiB without gaps; the
// 256 % K last lanes idle).  last: N, or 0 when every stage uses stage 0's set ("static_obstacles").
__global__ void __launch_bounds__(256) usv_obstacle_predict(const double2 *pos, const double2 *vel, double2 *p, int N, int K, int last, double dt)
{
    const int per = 256 / K; // (1 <= K <= 32)
    const int k0 = (int)threadIdx.x / K, i = (int)threadIdx.x - k0 * K;
    if (k0 >= per) return;
    const long b = blockIdx.x;
    const double2 q = pos[b * K + i], v = vel[b * K + i];
    double2 *row = p + b * (long)(N + 1) * K + i;
    for (int k = k0; k <= last; k += per) {
        double2 o;
        o.x = track_predict(q.x, v.x, k, dt);
        o.y = track_predict(q.y, v.y, k, dt);
        row[(long)k * K] = o;
    }
}

// usv_obstacle_step: the world moves on by T (pos += T vel), then the clearance the vehicle keeps - x0's position states (ipx, ipy) against
// the stepped obstacles and stage 0's lh - and its running minimum (reset: the minimum starts again).  One lane per instance.
__global__ void __launch_bounds__(256) usv_obstacle_step(double *pos, const double *vel, const double *x0, const double *lh, double *clear,
                                                         double *clear_min, int B, int K, int N, int nx, int ipx, int ipy, double T, int reset)
{
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (long)B) return;
    double *q = pos + b * 2 * K;
    const double *v = vel + b * 2 * K;
    for (int j = 0; j < 2 * K; j++) q[j] = track_step(q[j], v[j], T);
    const double c = track_clearance(x0[b * nx + ipx], x0[b * nx + ipy], q, lh + b * (long)N * K, K);
    clear[b] = c;
    const double m = clear_min[b];
    clear_min[b] = (reset || c < m) ? c : m;
}

// ---- Path-following front end (model usv_model_pf_ca; the arithmetic: pf_guidance.hpp).
constexpr int PF_GROUP = 64; // instances per workgroup of usv_pf_prepare

static __global__ void usv_pf_reset(PfPtrs F, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) *F.yref_writes = 0ull;
    if (b >= B) return;
    F.k[b] = 1; // main :394
    F.phase[b] = PF_SWITCH; // (nothing to publish yet)
    F.finish_tick[b] = -1;
    F.past[2 * b] = 0.0; F.past[2 * b + 1] = 0.0; // :172-173
    F.last[3 * b] = F.last[3 * b + 1] = F.last[3 * b + 2] = __builtin_nan("");
    F.u[b] = 0.0; F.ye[b] = 0.0;
    F.min_clear[b] = 1e300;
    F.min_sep[b] = 1e300; F.sep_tick[b] = -1;
    F.thr_port[b] = 0.0; F.thr_stbd[b] = 0.0; F.Tx[b] = 0.0; F.Tz[b] = 0.0; F.speed[b] = 0.0;
    F.e_u[b] = 0.0f; F.e_ye[b] = 0.0f;
    F.active[b] = 0;
}

// usv_pf_prepare: one workgroup per PF_GROUP consecutive instances, in two steps.
// 1. Decide: the first wave, one lane per instance - vessel state (host-fed arrays or x0 in place), waypoint manager, x0, the nearest-K
//    selection over the instance's world list (L <= 64; the distances in LDS, one column per lane) into stage 0 of p / lh, and whether the
//    instance's reference rows must be rewritten: only when (sin ak, cos ak, u_des) differ bit for bit from what it last wrote, or the caller
//    may have written yref (stale).  The triple and the decision go to LDS.  These are 14 + 3L + 3K doubles per instance: small, scattered.
// 2. Stream: the workgroup's yref rows are ONE contiguous run of PF_GROUP * N * 16 doubles (335 MB over 65 536 instances at N = 40 - the
//    reference rewrites it every tick).  All 256 threads walk it in 16-byte stores, thread t the t-th pair of each 4 KiB pass (a wave's stores
//    cover 1 KiB without gaps), skipping the instances that keep their rows; 256 % 8 == 0, so a thread always holds the same pair of a row and
//    only its instance moves on.  yref_e (7 pairs per instance) likewise.  No thread walks an instance's rows alone.
// A moving world (F.wvel: usvmpc_pf_world_vel, option "pf_predict" 1): the decide step selects as ever, on the current positions, but leaves each
// slot's TRACK (position pair, velocity pair, lh) in the [B][K] scratch F.trk_pv / F.trk_lh instead of writing stage 0, and between the two
// steps above comes
// 1b. Stream p and lh: the workgroup's instances own one contiguous run of p (PF_GROUP * (N + 1) * K pairs) and one of lh
//    (PF_GROUP * N * K doubles).  All 256 threads walk each in 16-byte stores, thread t the t-th pair of every 4 KiB pass, looking its slot's
//    track up again as (instance, stage, slot) moves on (K need not divide 256); the tracks of a wave's pass are a few hundred bytes the
//    workgroup itself has just written.  Instances whose mission is over keep their p and lh; switch ticks write.  A pair of lh that
//    straddles two instances of which one keeps its rows is stored as single doubles.
// With F.wvel null the kernel's stores are those of a world at rest: stage 0 only, by the deciding lane.
__global__ void __launch_bounds__(256) usv_pf_prepare(DevPtrs P, PfPtrs F, int tick, int stale)
{
    const DevSpec &S = *P.spec;
    const int B = S.B, N = S.N, K = S.K;
    __shared__ double s_d[PF_LMAX * PF_GROUP];
    __shared__ double s_ref[PF_GROUP][3];
    __shared__ int s_write[PF_GROUP];
    __shared__ unsigned s_count;
    __shared__ int s_obs[PF_GROUP]; // (a moving world: the instance's p / lh are written this tick)
    __shared__ unsigned s_nobs;
    const int t = (int)threadIdx.x;
    const long b0 = (long)blockIdx.x * PF_GROUP;
    const int cnt = (int)((long)B - b0 < (long)PF_GROUP ? (long)B - b0 : (long)PF_GROUP);
    if (t == 0) { s_count = 0u; s_nobs = 0u; }
    if (t < PF_GROUP) { s_write[t] = 0; s_obs[t] = 0; }
    __syncthreads();
    if (t < cnt) {
        const long b = b0 + t;
        double *x0 = const_cast<double *>(P.x0) + b * PF_NX;
        double u, v, r, psi, nedx, nedy, pp, ps;
        if (F.vel) {
            u = F.vel[3 * b]; v = F.vel[3 * b + 1]; r = F.vel[3 * b + 2];
            nedx = F.pose[3 * b]; nedy = F.pose[3 * b + 1]; psi = F.pose[3 * b + 2];
            pp = F.past[2 * b]; ps = F.past[2 * b + 1];
        } else { // as usv_advance / usv_advance_sim left it
            psi = x0[0]; u = x0[3]; v = x0[4]; r = x0[5]; nedx = x0[10]; nedy = x0[11]; pp = x0[12]; ps = x0[13];
        }
        u = pf_fix_u(u);
        const int k = F.k[b];
        PfSegment seg;
        const int phase = pf_waypoint(F.wp + b * 2 * F.npts, F.npts, k, nedx, nedy, seg);
        F.phase[b] = phase;
        if (phase == PF_SWITCH) F.k[b] = k + 1;
        if (phase == PF_OVER && F.finish_tick[b] < 0) F.finish_tick[b] = tick;
        if (phase != PF_OVER) {
            const int L = F.nworld < PF_LMAX ? F.nworld : PF_LMAX;
            double dmin;
            if (F.wvel) {
                dmin = pf_select_tracks(F.world + b * 3 * F.nworld, F.wvel + b * 2 * F.nworld, L, K, nedx, nedy, F.max_radius, F.margin, s_d + t,
                                        PF_GROUP, F.trk_pv + b * 4 * K, F.trk_lh + b * K, F.chosen ? F.chosen + b * K : nullptr);
                s_obs[t] = 1;
                atomicAdd(&s_nobs, 1u);
            } else {
                dmin = pf_select(F.world + b * 3 * F.nworld, L, K, nedx, nedy, F.max_radius, F.margin, s_d + t, PF_GROUP,
                                 const_cast<double *>(P.p) + b * (long)(N + 1) * 2 * K, const_cast<double *>(P.lh) + b * (long)N * K, nullptr);
            }
            if (dmin < F.min_clear[b]) F.min_clear[b] = dmin;
        } else if (F.chosen) { // (exchanged plans: an instance that does not stream has no slot a plan could feed)
            for (int s = 0; s < K; s++) F.chosen[b * K + s] = -1;
        }
        if (phase == PF_ACTIVE) {
            pf_x0(psi, u, v, r, seg, nedx, nedy, pp, ps, x0);
            F.u[b] = u; F.ye[b] = seg.ye;
        }
        double *last = F.last + 3 * b;
        if (pf_yref_write(phase, stale != 0, last, seg)) {
            last[0] = seg.sin_ak; last[1] = seg.cos_ak; last[2] = seg.u_des;
            s_ref[t][0] = seg.sin_ak; s_ref[t][1] = seg.cos_ak; s_ref[t][2] = seg.u_des;
            s_write[t] = 1;
            atomicAdd(&s_count, 1u);
        } else if (stale) {
            last[0] = last[1] = last[2] = __builtin_nan(""); // (rows the caller may have overwritten: rewritten at the instance's next active tick)
        }
    }
    __syncthreads();
    if (s_nobs != 0u && K > 0) {
        const double dt = S.dt;
        const double2 *pv = reinterpret_cast<const double2 *>(F.trk_pv) + b0 * 2 * K; // [cnt][K][2]: (X, Y), (vX, vY)
        {
            double2 *row = reinterpret_cast<double2 *>(const_cast<double *>(P.p)) + b0 * (long)(N + 1) * K;
            const int per = (N + 1) * K, total = cnt * per; // pairs per instance / of the workgroup
            int inst = 0, rem = t;                          // j = inst * per + rem
            while (rem >= per) { rem -= per; inst++; }
            for (int j = t; j < total; j += 256) {
                if (s_obs[inst]) {
                    const int k = rem / K, slot = rem - k * K;
                    const double2 q = pv[(inst * K + slot) * 2], v = pv[(inst * K + slot) * 2 + 1];
                    double2 o;
                    o.x = track_predict(q.x, v.x, k, dt);
                    o.y = track_predict(q.y, v.y, k, dt);
                    row[j] = o;
                }
                rem += 256;
                while (rem >= per) { rem -= per; inst++; }
            }
        }
        {
            double *row = const_cast<double *>(P.lh) + b0 * (long)N * K;
            const double *tl = F.trk_lh + b0 * K;
            const int per = N * K, total = cnt * per; // doubles per instance / of the workgroup
            int inst = 0, rem = 2 * t;                // e = 2 j = inst * per + rem: the pair's first double
            while (rem >= per) { rem -= per; inst++; }
            for (int e = 2 * t; e < total; e += 512) {
                int inst1 = inst, rem1 = rem + 1;     // its second
                if (rem1 == per) { rem1 = 0; inst1++; }
                const bool w0 = s_obs[inst] != 0, w1 = e + 1 < total && s_obs[inst1] != 0;
                const double a = w0 ? tl[inst * K + rem % K] : 0.0, c = w1 ? tl[inst1 * K + rem1 % K] : 0.0;
                if (w0 && w1) *reinterpret_cast<double2 *>(row + e) = double2{a, c};
                else if (w0) row[e] = a;
                else if (w1) row[e + 1] = c;
                rem += 512;
                while (rem >= per) { rem -= per; inst++; }
            }
        }
    }
    const unsigned nwrite = s_count;
    if (nwrite == 0u) return;
    if (t == 0) atomicAdd(F.yref_writes, (unsigned long long)nwrite);
    {
        double2 *row = reinterpret_cast<double2 *>(const_cast<double *>(P.yref)) + b0 * (long)N * (PF_NY / 2);
        const int per = N * (PF_NY / 2), total = cnt * per; // pairs per instance / of the workgroup
        const int pair = t & 7;
        int inst = 0, rem = t; // j = inst * per + rem
        while (rem >= per) { rem -= per; inst++; }
        for (int j = t; j < total; j += 256) {
            if (s_write[inst]) {
                double2 o;
                o.x = pf_yref_entry(2 * pair, s_ref[inst][0], s_ref[inst][1], s_ref[inst][2]);
                o.y = pf_yref_entry(2 * pair + 1, s_ref[inst][0], s_ref[inst][1], s_ref[inst][2]);
                row[j] = o;
            }
            rem += 256;
            while (rem >= per) { rem -= per; inst++; }
        }
    }
    {
        double2 *row = reinterpret_cast<double2 *>(const_cast<double *>(P.yref_e)) + b0 * (long)(PF_NX / 2);
        for (int j = t; j < cnt * (PF_NX / 2); j += 256) {
            const int inst = j / (PF_NX / 2), pair = j - inst * (PF_NX / 2);
            if (!s_write[inst]) continue;
            double2 o;
            o.x = pf_yref_entry(2 * pair, s_ref[inst][0], s_ref[inst][1], s_ref[inst][2]);
            o.y = pf_yref_entry(2 * pair + 1, s_ref[inst][0], s_ref[inst][1], s_ref[inst][2]);
            row[j] = o;
        }
    }
}

// usv_pf_world_step: the front end's world moves on by T, one thread per world entry (R is untouched)
__global__ void __launch_bounds__(256) usv_pf_world_step(double *world, const double *wvel, long n, double T)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pf_world_step(world + 3 * i, wvel + 2 * i, T);
}

// usv_pf_fleet_gather: vessel encounters (fleet_world.hpp) - the other S - 1 vessels of an instance's scene, as the plant left them in x0,
// become the fleet entries behind the n_fixed fixed ones of its world list.  A kernel of its own ahead of usv_pf_prepare, which rewrites
// x0[1..3] while a scene-mate in another workgroup would still be reading them; this one reads x0 only.  One thread per (instance, fleet
// slot), the slot fastest: a thread loads six doubles of one scene-mate (the scene's states are S neighbouring 112-byte rows) and stores one
// entry (24 bytes) and one velocity (16 bytes); the threads of an instance store its S - 1 entries as one run, a wave's runs lying
// 24 nworld bytes apart.  The separation bookkeeping needs all S - 1 distances of an instance in one place: its slot-0 thread takes the
// S - 1 positions again (lines its own wave has just loaded) - no atomics, no LDS.
// The body is the same for both front ends' models (usv_guidance_fleet_gather below): Fleet says how wide a state is and how an entry and a
// separation are made of it (fleet_world.hpp: PfFleet; ca_fleet_world.hpp: CaFleet).
template <class Fleet>
__device__ __forceinline__ void fleet_gather_body(const double *x0, double *world, double *wvel, double *min_sep, int *sep_tick, long B, int S,
                                                  int n_fixed, double radius, int tick)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = S - 1;
    if (t >= B * f) return;
    const long i = t / f;
    const int e = (int)(t - i * f);
    const long at = i * (n_fixed + f) + n_fixed + e; // the entry's place in the [B][nworld] lists
    Fleet::entry(x0 + fleet_vessel(i, e, S) * Fleet::NX, radius, world + 3 * at, wvel + 2 * at);
    if (e != 0) return;
    double m = min_sep[i];
    int mt = sep_tick[i];
    for (int q = 0; q < f; q++) fleet_closest(Fleet::separation(x0 + i * Fleet::NX, x0 + fleet_vessel(i, q, S) * Fleet::NX), tick, m, mt);
    min_sep[i] = m;
    sep_tick[i] = mt;
}

__global__ void __launch_bounds__(256) usv_pf_fleet_gather(const double *x0, double *world, double *wvel, double *min_sep, int *sep_tick,
                                                           long B, int S, int n_fixed, double radius, int tick)
{
    fleet_gather_body<PfFleet>(x0, world, wvel, min_sep, sep_tick, B, S, n_fixed, radius, tick);
}

// usv_pf_publish: the node's outputs after the solve, one lane per instance (a dozen scalars each).  An active instance reads the thrusters
// from x_1 and keeps them as its past thrust; one whose mission is over publishes zero thrust and speed; a switch tick publishes nothing.
__global__ void __launch_bounds__(256) usv_pf_publish(DevPtrs P, PfPtrs F)
{
    const DevSpec &S = *P.spec;
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (long)S.B) return;
    const int phase = F.phase[b];
    F.active[b] = phase == PF_ACTIVE ? 1 : 0;
    if (phase == PF_ACTIVE) {
        const double *x1 = P.x + (b * (S.N + 1) + 1) * PF_NX;
        PfOutputs o;
        pf_publish(x1[12], x1[13], PF_SPEED, F.u[b], F.ye[b], o);
        F.thr_port[b] = o.thr_port; F.thr_stbd[b] = o.thr_stbd; F.Tx[b] = o.Tx; F.Tz[b] = o.Tz; F.speed[b] = o.speed;
        F.e_u[b] = o.e_u; F.e_ye[b] = o.e_ye;
        F.past[2 * b] = o.thr_port; F.past[2 * b + 1] = o.thr_stbd; // :359-360
    } else if (phase == PF_OVER) { // :260-266
        F.thr_port[b] = 0.0; F.thr_stbd[b] = 0.0; F.speed[b] = 0.0;
    }
}

// ---- Guidance front end, device-resident (model usv_model_guidance_ca1; the arithmetic: ca_guidance.hpp; host-fed kernels: guidance.hpp).
constexpr int CA_GROUP = 64; // instances per workgroup of usv_guidance_tick

// "none yet": a running minimum and the tick it was met at (the mission's clearance and finish tick, a fleet's separation)
static __global__ void usv_guidance_none_yet(double *minimum, int *tick, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    minimum[b] = 1e300;
    tick[b] = -1;
}

// usv_guidance_fleet_gather: vessel encounters (ca_fleet_world.hpp) - the other S - 1 vessels of an instance's scene, as the plant left them
// in x0, become the fleet entries behind the n_fixed fixed ones of its world list.  A kernel of its own ahead of usv_guidance_tick, which
// rewrites x0 (ca_x0) while a scene-mate in another workgroup would still be reading it; this one reads x0 only and writes the world lists
// and the separation bookkeeping only - nothing a lineariser reads.  Threads and stores as usv_pf_fleet_gather (one body, fleet_gather_body);
// a thread loads five doubles of one scene-mate (the scene's states are S neighbouring 64-byte rows) and takes one sine and one cosine.
__global__ void __launch_bounds__(256) usv_guidance_fleet_gather(const double *x0, double *world, double *wvel, double *min_sep, int *sep_tick,
                                                                 long B, int S, int n_fixed, double radius, int tick)
{
    fleet_gather_body<CaFleet>(x0, world, wvel, min_sep, sep_tick, B, S, n_fixed, radius, tick);
}

// usv_guidance_tick: the node's input side for a vessel whose state is the solver's own x0 (as usv_advance / usv_advance_sim left it) against
// a world list that lives on the device.  One workgroup per CA_GROUP consecutive instances, laid out as usv_pf_prepare:
// 1. Decide: the first wave, one lane per instance - (u, v) = x0[0..1], (nedx, nedy, psi) = x0[5..7]; the simulator's visibility test and
//    NED -> body transform per world entry (L <= 64; the body-frame list is never stored), the ranking distance of each visible entry ONCE
//    into LDS ([64 entries][64 lanes]: a lane walks its own column, consecutive lanes consecutive words - no bank conflict), the nearest-K
//    choice by comparisons, body -> NED through float32 for the chosen ones, the running minimum clearance, the waypoint manager, x0.  An
//    instance whose mission was over before this tick (k >= npts) keeps its x0, p and lh and is skipped altogether; the tick that ends a
//    mission still writes p and lh (as usv_guidance_pre does) and records finish_tick.  World at rest: the deciding lane stores stage 0.
// 2. Stream (W.wvel: a moving world that is predicted): the decide step left each slot's TRACK (float32-rounded NED position, the chosen
//    entry's velocity, lh) in the [B][K] scratch W.trk_pv / W.trk_lh.  The workgroup's instances own one contiguous run of p
//    (CA_GROUP * (N + 1) * K pairs) and one of lh (CA_GROUP * N * K doubles).  All 256 threads walk each in 16-byte stores, thread t the t-th
//    pair of every 4 KiB pass (a wave's stores cover 1 KiB without gaps), looking the slot's track up again as (instance, stage, slot) moves
//    on; skipped instances keep their rows, and a pair of lh that straddles a skipped instance is stored as single doubles.
__global__ void __launch_bounds__(256) usv_guidance_tick(DevPtrs P, GuidancePtrs G, CaTickPtrs W)
{
    const DevSpec &S = *P.spec;
    const int B = S.B, N = S.N, K = S.K;
    __shared__ double s_d[GUIDANCE_LMAX * CA_GROUP];
    __shared__ int s_obs[CA_GROUP]; // (the instance's p / lh are streamed this tick)
    __shared__ unsigned s_nobs;
    const int t = (int)threadIdx.x;
    const long b0 = (long)blockIdx.x * CA_GROUP;
    const int cnt = (int)((long)B - b0 < (long)CA_GROUP ? (long)B - b0 : (long)CA_GROUP);
    if (t == 0) s_nobs = 0u;
    if (t < CA_GROUP) s_obs[t] = 0;
    __syncthreads();
    if (t < cnt) {
        const long b = b0 + t;
        int k = G.k[b];
        if (k >= G.npts) { // the mission was over before this tick
            if (W.finish_tick[b] < 0) W.finish_tick[b] = W.tick;
            if (W.chosen) // (exchanged plans: an instance that does not stream has no slot a plan could feed)
                for (int s = 0; s < K; s++) W.chosen[b * K + s] = -1;
        } else {
            double *x0 = const_cast<double *>(P.x0) + b * CA_NX;
            const double u_cb = ca_fix_u(x0[0]), v_cb = x0[1], nedx = x0[5], nedy = x0[6], psi = x0[7];
            const int L = W.nworld < GUIDANCE_LMAX ? W.nworld : GUIDANCE_LMAX;
            const double *w = W.world + b * 3 * W.nworld;
            if (W.wvel) {
                ca_select_tracks(w, W.wvel + b * 2 * W.nworld, L, K, psi, nedx, nedy, W.max_radius, s_d + t, CA_GROUP, W.trk_pv + b * 4 * K,
                                 W.trk_lh + b * K, W.chosen ? W.chosen + b * K : nullptr);
                s_obs[t] = 1;
                atomicAdd(&s_nobs, 1u);
            } else {
                ca_select_world(w, L, K, psi, nedx, nedy, W.max_radius, s_d + t, CA_GROUP, const_cast<double *>(P.p) + b * (long)(N + 1) * 2 * K,
                                const_cast<double *>(P.lh) + b * (long)N * K, nullptr);
            }
            const double c = ca_min_clearance(w, L, nedx, nedy, s_d + t, CA_GROUP);
            if (c < W.min_clear[b]) W.min_clear[b] = c;
            float pp = G.past_psied[b];
            int active;
            double ak, ye;
            ca_waypoint(G.wp + b * 2 * G.npts, G.npts, nedx, nedy, k, pp, active, ak, ye);
            G.k[b] = k;
            G.active[b] = active;
            if (active) {
                G.past_psied[b] = pp;
                G.ak[b] = ak;
                G.ye[b] = ye;
                ca_x0(u_cb, v_cb, ye, psi, ak, pp, nedx, nedy, x0);
            } else if (W.finish_tick[b] < 0) {
                W.finish_tick[b] = W.tick;
            }
        }
    }
    __syncthreads();
    if (s_nobs == 0u || K <= 0) return;
    const double dt = S.dt;
    const double2 *pv = reinterpret_cast<const double2 *>(W.trk_pv) + b0 * 2 * K; // [cnt][K][2]: (X, Y), (vX, vY)
    {
        double2 *row = reinterpret_cast<double2 *>(const_cast<double *>(P.p)) + b0 * (long)(N + 1) * K;
        const int per = (N + 1) * K, total = cnt * per; // pairs per instance / of the workgroup
        int inst = 0, rem = t;                          // j = inst * per + rem
        while (rem >= per) { rem -= per; inst++; }
        for (int j = t; j < total; j += 256) {
            if (s_obs[inst]) {
                const int k = rem / K, slot = rem - k * K;
                const double2 q = pv[(inst * K + slot) * 2], v = pv[(inst * K + slot) * 2 + 1];
                double2 o;
                o.x = track_predict(q.x, v.x, k, dt);
                o.y = track_predict(q.y, v.y, k, dt);
                row[j] = o;
            }
            rem += 256;
            while (rem >= per) { rem -= per; inst++; }
        }
    }
    {
        double *row = const_cast<double *>(P.lh) + b0 * (long)N * K;
        const double *tl = W.trk_lh + b0 * K;
        const int per = N * K, total = cnt * per; // doubles per instance / of the workgroup
        int inst = 0, rem = 2 * t;                // e = 2 j = inst * per + rem: the pair's first double
        while (rem >= per) { rem -= per; inst++; }
        for (int e = 2 * t; e < total; e += 512) {
            int inst1 = inst, rem1 = rem + 1;     // its second
            if (rem1 == per) { rem1 = 0; inst1++; }
            const bool w0 = s_obs[inst] != 0, w1 = e + 1 < total && s_obs[inst1] != 0;
            const double a = w0 ? tl[inst * K + rem % K] : 0.0, c = w1 ? tl[inst1 * K + rem1 % K] : 0.0;
            if (w0 && w1) *reinterpret_cast<double2 *>(row + e) = double2{a, c};
            else if (w0) row[e] = a;
            else if (w1) row[e + 1] = c;
            rem += 512;
            while (rem >= per) { rem -= per; inst++; }
        }
    }
}

// ---- Exchanged plans (usvmpc_pf_fleet_plans / usvmpc_guidance_fleet_plans; the arithmetic: fleet_plan.hpp).  Enqueued behind a predicted
// prepare on the same stream when the handle's plan state says the iterate is one hand-over old (world_plan.hpp: plan_usable): the prepare
// has written every stage of p from the constant-velocity tracks; this kernel rewrites stages 1 .. N of the slots that hold a scene-mate
// with a usable plan, and nothing else.  A kernel of its own because a mate's finish_tick is written by another workgroup's decide step.
// One workgroup per 64 consecutive instances, the prepare's groups (PF_GROUP, CA_GROUP):
// 1. Sources: thread t takes the (instance, slot) pairs t, t + 256, .. of the group's [cnt][K] - the decide step's choice, the mate's
//    finish_tick and status - into LDS and into `source`; the plan-fed pairs are counted, one atomic per workgroup (as yref_writes).
// 2. Stream: the group's run of p (cnt * (N + 1) * K pairs) is walked as the prepare's stream step walks it, thread t the t-th pair of
//    every 4 KiB pass, but ONLY pairs whose slot has a source are stored: 16 bytes each, the others are not touched.
// The mates' position columns are 16 bytes of every 112- or 64-byte row of x and are read straight from memory, not staged in LDS.  The
// pairs of one pass that read the same row are neighbours in the pass (the S - 1 mates of a vessel hold it in one stage each, and their
// instances are adjacent), so the re-reads hit the line the first read brought into the CU's vector cache, and at the worst L2; HBM sees
// each line once either way.  A scene's columns in LDS would be (64 + 2 (S - 2)) (N + 1) 16 bytes per group - 107 KB at N = 100, one
// workgroup per CU - bought with a barrier and a second pass over the same lines, to save cache hits.  
constexpr int PLAN_GROUP = 64;
static_assert(PLAN_GROUP == PF_GROUP && PLAN_GROUP == CA_GROUP, "the plan kernel owns the prepare's groups");

struct FleetPlanArgs {
    const double *x;         // [B][N + 1][NX] the iterate
    const int *status;       // [B] of the last solve
    const int *finish_tick;  // [B] as this prepare left it
    const int *chosen;       // [B][K] the decide step's choice
    const double *trk_pv;    // [B][K][4] the slot tracks
    double *p;               // [B][N + 1][2K]
    int *source;             // [B][K] out: the vessel behind each plan-fed slot, -1: none
    unsigned long long *fed; // [1] plan-fed (instance, slot) pairs so far
    int B, N, K, S, n_fixed;
};

template <class Fleet>
__device__ __forceinline__ void fleet_plan_body(const FleetPlanArgs &A)
{
    const int N = A.N, K = A.K;
    __shared__ int s_src[PLAN_GROUP * KMAX];
    __shared__ unsigned s_fed;
    const int t = (int)threadIdx.x;
    const long b0 = (long)blockIdx.x * PLAN_GROUP;
    const int cnt = (int)((long)A.B - b0 < (long)PLAN_GROUP ? (long)A.B - b0 : (long)PLAN_GROUP);
    if (t == 0) s_fed = 0u;
    __syncthreads();
    unsigned mine = 0u;
    for (int e = t; e < cnt * K; e += 256) {
        const long i = b0 + e / K;
        long j = fleet_plan_source(i, A.chosen[b0 * K + e], A.n_fixed, A.S, A.finish_tick, A.status);
        if (j >= (long)A.B) j = -1; // (never: the batch is a whole number of scenes)
        s_src[e] = (int)j;
        A.source[b0 * K + e] = (int)j;
        mine += j >= 0 ? 1u : 0u;
    }
    if (mine) atomicAdd(&s_fed, mine);
    __syncthreads();
    if (s_fed == 0u) return;
    if (t == 0) atomicAdd(A.fed, (unsigned long long)s_fed);
    const double2 *pv = reinterpret_cast<const double2 *>(A.trk_pv) + b0 * 2 * K; // [cnt][K][2]: (X, Y), (vX, vY)
    double2 *row = reinterpret_cast<double2 *>(A.p) + b0 * (long)(N + 1) * K;
    const int per = (N + 1) * K, total = cnt * per; // pairs per instance / of the workgroup
    int inst = 0, rem = t;                          // j = inst * per + rem
    while (rem >= per) { rem -= per; inst++; }
    for (int j = t; j < total; j += 256) {
        const int k = rem / K, slot = rem - k * K;
        const int src = s_src[inst * K + slot];
        if (src >= 0 && k >= 1) {
            const double2 q = pv[(inst * K + slot) * 2];
            double2 o;
            fleet_plan_pair<Fleet>(A.x + (long)src * (N + 1) * Fleet::NX, N, k, q.x, q.y, o.x, o.y);
            row[j] = o;
        }
        rem += 256;
        while (rem >= per) { rem -= per; inst++; }
    }
}

__global__ void __launch_bounds__(256) usv_pf_fleet_plans(FleetPlanArgs A) { fleet_plan_body<PfFleet>(A); }
__global__ void __launch_bounds__(256) usv_guidance_fleet_plans(FleetPlanArgs A) { fleet_plan_body<CaFleet>(A); }

// ---- The two-layer control stack (usvmpc_cascade_*; the arithmetic: cascade.hpp): guidance layer -> low-level NMPC -> vessel.
constexpr int CAS_GROUP = 64; // instances per workgroup of usv_cascade_refs

static __global__ void usv_cascade_reset(CascadePtrs C, const double *pose, const double *vel, double *gx0, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) *C.yref_writes = 0ull;
    if (b >= B) return;
    double *s = C.s + (long)b * CAS_NS;
    s[0] = pose[3 * b]; s[1] = pose[3 * b + 1]; s[2] = pose[3 * b + 2];
    s[3] = vel[3 * b]; s[4] = vel[3 * b + 1]; s[5] = vel[3 * b + 2];
    C.thr[2 * b] = 0.0; C.thr[2 * b + 1] = 0.0;
    C.past[2 * b] = 0.0; C.past[2 * b + 1] = 0.0;
    C.last[2 * b] = cas_never(); C.last[2 * b + 1] = cas_never();
    C.ticks[b] = 0;
    C.sums[4 * b] = C.sums[4 * b + 1] = C.sums[4 * b + 2] = C.sums[4 * b + 3] = 0.0;
    double *x0 = gx0 + (long)b * CA_NX; // the entries usv_guidance_tick and usv_guidance_fleet_gather read
    x0[0] = s[3]; x0[1] = s[4]; x0[5] = s[0]; x0[6] = s[1]; x0[7] = s[2];
}

// usv_cascade_refs: the low-level node's input side.  One workgroup per CAS_GROUP consecutive instances, laid out as usv_pf_prepare:
// 1. Decide: the first wave, one lane per instance - the low-level x0 (eight doubles) from the vessel's state and the past thrusts, the
//    guidance layer's published (heading, speed), and whether the instance's reference rows must be rewritten: only when the bits of the pair
//    differ from what it last wrote.  One sine and one cosine per rewritten instance, by this lane; the row's four values go to LDS.
// 2. Stream: the workgroup's yref rows are ONE contiguous run of CAS_GROUP * ll_N * 10 doubles (524 MB over 65 536 instances at N = 100, on
//    every guidance tick: the heading moves every tick).  All 256 threads walk it in 16-byte stores, thread t the t-th pair of each 4 KiB
//    pass (a wave's stores cover 1 KiB without gaps), skipping the instances that keep their rows.  yref_e (4 pairs per instance) likewise.
// It writes memory of ANOTHER library's solver (CascadePtrs): that solver must linearise afresh from device memory at every solve.
__global__ void __launch_bounds__(256) usv_cascade_refs(GuidancePtrs G, CascadePtrs C, int B)
{
    __shared__ double s_ref[CAS_GROUP][4];
    __shared__ int s_write[CAS_GROUP];
    __shared__ unsigned s_count;
    const int t = (int)threadIdx.x, N = C.ll_N;
    const long b0 = (long)blockIdx.x * CAS_GROUP;
    const int cnt = (int)((long)B - b0 < (long)CAS_GROUP ? (long)B - b0 : (long)CAS_GROUP);
    if (t == 0) s_count = 0u;
    if (t < CAS_GROUP) s_write[t] = 0;
    __syncthreads();
    if (t < cnt) {
        const long b = b0 + t;
        cas_ll_x0(C.s + b * CAS_NS, C.past + 2 * b, C.ll_x0 + b * CAS_NX);
        const double psi_des = G.heading[b], u_des = G.speed[b];
        double *last = C.last + 2 * b;
        if (cas_ref_changed(last, psi_des, u_des)) {
            const CasRef r = cas_ref(psi_des, u_des);
            last[0] = psi_des; last[1] = u_des;
            s_ref[t][0] = r.psi; s_ref[t][1] = r.s; s_ref[t][2] = r.c; s_ref[t][3] = r.u;
            s_write[t] = 1;
            atomicAdd(&s_count, 1u);
        }
    }
    __syncthreads();
    const unsigned nwrite = s_count;
    if (nwrite == 0u) return;
    if (t == 0) atomicAdd(C.yref_writes, (unsigned long long)nwrite);
    {
        double2 *row = reinterpret_cast<double2 *>(C.ll_yref) + b0 * (long)N * (CAS_NY / 2);
        const int per = N * (CAS_NY / 2), total = cnt * per; // pairs per instance / of the workgroup
        int inst = 0, rem = t; // j = inst * per + rem
        while (rem >= per) { rem -= per; inst++; }
        for (int j = t; j < total; j += 256) {
            if (s_write[inst]) {
                const int pair = rem % (CAS_NY / 2);
                const CasRef r = {s_ref[inst][0], s_ref[inst][1], s_ref[inst][2], s_ref[inst][3]};
                double2 o;
                o.x = cas_yref_entry(2 * pair, r);
                o.y = cas_yref_entry(2 * pair + 1, r);
                row[j] = o;
            }
            rem += 256;
            while (rem >= per) { rem -= per; inst++; }
        }
    }
    {
        double2 *row = reinterpret_cast<double2 *>(C.ll_yref_e) + b0 * (long)(CAS_NX / 2);
        for (int j = t; j < cnt * (CAS_NX / 2); j += 256) {
            const int inst = j / (CAS_NX / 2), pair = j - inst * (CAS_NX / 2);
            if (!s_write[inst]) continue;
            const CasRef r = {s_ref[inst][0], s_ref[inst][1], s_ref[inst][2], s_ref[inst][3]};
            double2 o;
            o.x = cas_yref_entry(2 * pair, r);
            o.y = cas_yref_entry(2 * pair + 1, r);
            row[j] = o;
        }
    }
}

// usv_cascade_step: the low-level node's output side and the vessel.  One lane per instance: thrusts and past thrusts from stage 1 of the
// low-level iterate, the errors against the state the solve saw, one plant period under the published thrusts, the optional disturbance on
// (u, v, r) - keyed by the instance's GLOBAL index, as usv_advance -, and, when the NEXT low-level tick is a guidance tick (hand_over), the
// vessel's state into the guidance solver's x0[0, 1, 5, 6, 7]: the entries usv_guidance_tick and usv_guidance_fleet_gather read, nothing a
// lineariser reads.
__global__ void __launch_bounds__(256) usv_cascade_step(CascadePtrs C, double *gx0, int B, double T, int steps, double c, double sigma,
                                                        unsigned long long seed, long long offset, int hand_over)
{
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (long)B) return;
    const double *x1 = C.ll_x + (b * (long)(C.ll_N + 1) + 1) * CAS_NX;
    double s[CAS_NS], thr[2], past[2];
    sfor<0, CAS_NS>([&](auto i) { s[i] = C.s[b * CAS_NS + i]; });
    float e_u, e_psi;
    cas_ll_outputs(x1, C.last[2 * b], C.last[2 * b + 1], s[2], cas_fix_u(s[3]), thr, past, e_u, e_psi);
    C.thr[2 * b] = thr[0]; C.thr[2 * b + 1] = thr[1];
    C.past[2 * b] = past[0]; C.past[2 * b + 1] = past[1];
    {
        double *sm = C.sums + 4 * b;
        const double eu = (double)e_u, ep = (double)e_psi;
        sm[0] = track_add(sm[0], fabs(eu)); sm[1] = track_add(sm[1], fabs(ep));
        sm[2] = track_add(sm[2], track_mul(eu, eu)); sm[3] = track_add(sm[3], track_mul(ep, ep));
    }
    cas_plant_period(s, thr, c, T, steps);
    if (sigma != 0.0) sfor<3, CAS_NS>([&](auto j) { s[j] += noise(sigma, seed, (unsigned long long)((offset + b) * CAS_NS + j)); });
    sfor<0, CAS_NS>([&](auto i) { C.s[b * CAS_NS + i] = s[i]; });
    C.ticks[b] += 1;
    if (hand_over) {
        double *x0 = gx0 + b * CA_NX;
        x0[0] = s[3]; x0[1] = s[4]; x0[5] = s[0]; x0[6] = s[1]; x0[7] = s[2];
    }
}

// usv_cascade_record: one launch per logged low-level tick (usvmpc_cascade_log_*; the schedule and layout: cascade_log_plan.hpp), enqueued
// AHEAD of usv_cascade_step, so that C.s is still the state the tick's low-level solve saw and stage 1 of its iterate is final.  It reads
// the cascade's state, the low-level iterate and both solvers' status and writes log memory only.  Shaped like usv_log_record: thread t
// serves element t of each of the record's five slabs (five guards), so every store of a wave is one contiguous run; the selected states
// travel as a nibble list in one 64-bit argument and nothing in the argument struct is indexed at run time (that kernel's scratch trap).
// Thrusts and errors come from cas_ll_outputs on the very arguments usv_cascade_step hands it: the recorded bits are the published bits.
__global__ void __launch_bounds__(256) usv_cascade_record(CasLogRec R)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (R.r_state && t < R.B * R.nsel) {
        const long b = t / R.nsel;
        const int j = (int)(t - b * R.nsel);
        R.r_state[t] = R.s[b * CAS_NS + log_nibble(R.sel, j)];
    }
    if ((R.r_thrust || R.r_err) && t < 2 * R.B) {
        const long b = t >> 1;
        const bool second = (t & 1) != 0;
        const double *x1 = R.ll_x + (b * (long)(R.ll_N + 1) + 1) * CAS_NX;
        double thr[2], past[2];
        float e_u, e_psi;
        cas_ll_outputs(x1, R.last[2 * b], R.last[2 * b + 1], R.s[b * CAS_NS + 2], cas_fix_u(R.s[b * CAS_NS + 3]), thr, past, e_u, e_psi);
        if (R.r_thrust) R.r_thrust[t] = second ? thr[1] : thr[0];
        if (R.r_err) R.r_err[t] = second ? e_psi : e_u;
    }
    if (R.r_ref && t < 2 * R.B) R.r_ref[t] = R.last[t];
    if (R.r_status && t < R.B) R.r_status[t] = cas_log_status_word(R.ll_status[t], R.ll_qp_iter[t], R.g_status[t], R.g_qp_iter[t]);
}

// AcadosSimSolver's solve (usvmpc_sim_solve): x, u -> x_next (and S_forw = [Sx | Su] when SENS), sim.hpp
template <class M, bool SENS>
__global__ void __launch_bounds__(256) usv_sim(const double *x, const double *u, double *xn, double *S, long B, double T, int steps)
{
    sim_run<M, SENS>(x, u, xn, S, B, T, steps);
}

// Debug / test entry points: the model functions exactly as the lineariser calls them (M::fjvp: f and one Jacobian
// column per call) and the obstacle-row geometry exactly as the QP kernel evaluates it (obs_dist), on caller-supplied
// points, so that a GPU test can compare the device transcription with vectors derived from the reference's own
// model files (tests/golden/ref_model_*.npz).  One thread per (point, column).
template <class M>
__global__ void usv_debug_model(int n, const double *x, const double *u, double *f, double *J)
{
    constexpr int NX = M::NX, NU = M::NU, NZ = NX + NU;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * NZ) return;
    const int pt = i / NZ, c = i - pt * NZ;
    double xx[NX], uu[NU > 0 ? NU : 1], s[NX], su[NU > 0 ? NU : 1], ff[NX], js[NX];
    for (int j = 0; j < NX; j++) { xx[j] = x[pt * NX + j]; s[j] = (c == NU + j) ? 1.0 : 0.0; }
    for (int j = 0; j < NU; j++) { uu[j] = u[pt * NU + j]; su[j] = (c == j) ? 1.0 : 0.0; }
    M::fjvp(xx, uu, s, su, ff, js);
    for (int j = 0; j < NX; j++) {
        J[((long)pt * NX + j) * NZ + c] = js[j];   // d f_j / d z_c, z = [u; x]
        if (c == 0) f[pt * NX + j] = ff[j];
    }
}

// ... and as the lineariser and the integrator call them INSIDE an interval: ModelCall<M>::prepare at the interval's start x_start, then
// ModelCall<M>::fjvp at the point x.  For a model with a Pre (ModelM2) this evaluates what depends on the distance from the start -
// sincos_near at d = x[0] - x_start[0] - which usv_debug_model, preparing at the point itself, never enters.
template <class M>
__global__ void usv_debug_model_from(int n, const double *x_start, const double *x, const double *u, double *f, double *J)
{
    constexpr int NX = M::NX, NU = M::NU, NZ = NX + NU;
    using MC = ModelCall<M>;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * NZ) return;
    const int pt = i / NZ, c = i - pt * NZ;
    double x0[NX], xx[NX], uu[NU > 0 ? NU : 1], s[NX], su[NU > 0 ? NU : 1], ff[NX], js[NX];
    for (int j = 0; j < NX; j++) { x0[j] = x_start[pt * NX + j]; xx[j] = x[pt * NX + j]; s[j] = (c == NU + j) ? 1.0 : 0.0; }
    for (int j = 0; j < NU; j++) { uu[j] = u[pt * NU + j]; su[j] = (c == j) ? 1.0 : 0.0; }
    const typename MC::Pre pre = MC::prepare(x0);
    MC::fjvp(pre, xx, uu, s, su, ff, js);
    for (int j = 0; j < NX; j++) {
        J[((long)pt * NX + j) * NZ + c] = js[j];
        if (c == 0) f[pt * NX + j] = ff[j];
    }
}

// lanes::frcp and lanes::frsqrt on caller-supplied operands, one thread per operand
__global__ void usv_debug_fast_math(int n, const double *x, double *rcp, double *rsq)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rcp[i] = lanes::frcp(x[i]);
    rsq[i] = lanes::frsqrt(x[i]);
}

__global__ void usv_debug_obstacle(int n, int K, const double *pos, const double *p, double *h, double *grad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * K) return;
    const int pt = i / K, k = i - pt * K;
    double d, ux, uy;
    usv::obs_dist(pos[2 * pt] - p[(long)pt * 2 * K + 2 * k], pos[2 * pt + 1] - p[(long)pt * 2 * K + 2 * k + 1], d, ux, uy);
    h[i] = d; grad[2 * i] = ux; grad[2 * i + 1] = uy;
}

// Every primitive of lanes.hpp on caller-supplied operands (lanes_probe.hpp: the same body runs on the CPU emulator of the test suite):
// a workgroup of WAVES waves takes 4 * WAVES groups, one per 16-lane row
template <int WAVES>
__global__ void __launch_bounds__(WAVES * 64) usv_debug_lanes(lanes_probe::Args a)
{
    lanes_probe::run<WAVES>(a, (long)blockIdx.x * (long)(4 * WAVES));
}

// Traffic calibration for the rocprofv3 FETCH_SIZE / WRITE_SIZE counters: streams a KNOWN number of
// workspace planes with exactly the access instruction of the solver kernels (one
// buffer_load_dwordx2 per lane per plane, 16 lanes of a group contiguous) and writes one plane.
__global__ void __launch_bounds__(64) usv_calib_stream(DevPtrs P, long ngroups, int nread)
{
    const long g = lanes::group_linear();
    if (g >= ngroups) return;
    const lanes::Planes W(P.ws, (unsigned)(ngroups * (nread + 1) * 128), lanes::Planes::lane_offset(g, nread + 1, lanes::lane()));
    double acc = 0.0;
    for (int i = 0; i < nread; i++) acc += W.ld(i);
    W.st(nread, acc);
}
#endif // USV_MAIN

// Difficulty binning: a wave carries four instances and runs until the slowest one converges, so
// instances are grouped by the IPM iteration count of their previous solve (a counting sort on the
// device, hardest first so that long-running waves start early).  Only the group -> instance map
// changes; the arithmetic of an instance does not depend on its neighbours.
constexpr int SORT_BINS = 64;

// (histogram and ranks are formed per workgroup in LDS; a workgroup then touches each global bin once - 65 536 threads
// hammering 64 global counters took 0.19 ms per kernel)
// The sort key of an instance: its IPM iteration count in the last solve - or, option "sort_two_ticks", the larger of the last TWO.
// What the launch must avoid is an instance that runs long being handed out late (it then ends with a few waves finishing it while
// the device idles: a tenth of the launch on the bench workload); one tick's count predicts the next with correlation 0.53 only.
// The two-tick key looked better in schedule simulations and measured the same on the device (profiles/r03_tail.txt): off by default.
__device__ __forceinline__ int sort_key(const int *qp_iter, const int *qp_iter_prev, int i)
{
    return min(max(max(qp_iter[i], qp_iter_prev[i]), 0), SORT_BINS - 1);
}

static __global__ void __launch_bounds__(256) usv_sort_hist(const int *qp_iter, const int *qp_iter_prev, int B, int *hist)
{
    __shared__ int loc[SORT_BINS];
    if (threadIdx.x < SORT_BINS) loc[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) atomicAdd(&loc[sort_key(qp_iter, qp_iter_prev, i)], 1);
    __syncthreads();
    if (threadIdx.x < SORT_BINS && loc[threadIdx.x] != 0) atomicAdd(&hist[threadIdx.x], loc[threadIdx.x]);
}

static __global__ void usv_sort_scan(int *hist, int *cursor)
{
    if (threadIdx.x == 0) {
        int pos = 0;
        for (int b = SORT_BINS - 1; b >= 0; b--) { // descending difficulty
            cursor[b] = pos;
            pos += hist[b];
            hist[b] = 0;
        }
    }
}

// (inv: the inverse map, instance -> group, for the speculative lineariser's work order - lin_order.hpp; nullptr: not wanted)
static __global__ void __launch_bounds__(256) usv_sort_scatter(const int *qp_iter, const int *qp_iter_prev, int B, int *cursor, int *perm, int *inv)
{
    __shared__ int loc[SORT_BINS], base[SORT_BINS];
    if (threadIdx.x < SORT_BINS) loc[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int bin = 0, rank = 0;
    if (i < B) {
        bin = sort_key(qp_iter, qp_iter_prev, i);
        rank = atomicAdd(&loc[bin], 1);
    }
    __syncthreads();
    if (threadIdx.x < SORT_BINS && loc[threadIdx.x] != 0) base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], loc[threadIdx.x]);
    __syncthreads();
    if (i < B) {
        perm[base[bin] + rank] = i;
        if (inv) inv[i] = base[bin] + rank;
    }
}

// instance -> group from group -> instance (option "lin_force_modes": the map of a solve that no sort of its own launch made)
static __global__ void __launch_bounds__(256) usv_invert_map(const int *perm, int B, int *inv)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < B) inv[perm[g]] = g;
}

// ---------------------------------------------------------------------------------- handle
struct usvmpc_handle {
    usvmpc_desc desc;
    DevSpec spec;
    DevPtrs ptrs;
    int nx, nu, nz, ny, ny_e, N, K, B, Bp, kch;
    bool soft;
    int device;
    hipStream_t stream;
    bool own_stream = true;
    Options opt;              // the run-time options (option_plan.hpp: the table of their names, checks and effects; usvmpc_set_option)
    static constexpr int RING = 64;      // per-solve event triples, newest at (nsolves-1) % RING
    hipEvent_t ev[RING][4];   // start | lineariser done | QP phase done | main QP launch done (the follow-up launch of a hand-over comes after it)
    long nsolves;
    DevSpec *d_spec;
    int *d_perm, *d_hist, *d_cursor, *d_iter_prev;
    GuidancePtrs gd;          // device buffers of the guidance front end (allocated on first use)
    bool gd_ready;
    int gd_npts_cap;
    double *gd_psi;
    double *gd_sense_world;   // [B][n_world][3] the host-fed world obstacles of the last usvmpc_guidance_sense (not the resident list: `world`)
    size_t gd_sense_world_cap;
    // Path-following front end (usvmpc_pf_*, model usv_model_pf_ca): device buffers on first use; pf_ready after usvmpc_pf_reset
    PfPtrs pf;
    bool pf_alloc, pf_ready;
    bool pf_stale = true;     // the caller may have written yref / yref_e since the front end last did: the next prepare rewrites every active instance
    int pf_tick;              // prepares since the last reset
    int pf_npts_cap;
    double *pf_vel, *pf_pose; // [B][3] staging of the host-fed mode
    // The front end's resident world (usvmpc_guidance_world / usvmpc_pf_world and their _world_vel, _world_step, _world_read, _fleet and
    // _fleet_state): a handle has one model, so one front end and ONE world.  What a call refuses, what it does and what the list is afterwards
    // is world_plan.hpp's: the state machine WorldPlan (no field of it is assigned in this file - the entry points ask it to judge, carry_world
    // does what it answers and commits), host-only and checked on the CPU by tests/test_world_plan.py.  Here: the device buffers it speaks of.
    // The world members of PfPtrs / CaTickPtrs (kernel arguments) are filled from these where a launch is made: pf_args, guidance_tick.
    WorldPlan world;
    struct WorldBufs {
        double *list;         // [B][nworld][3] NED (X, Y, R): the caller's fixed entries, a fleet's slots behind them (fleet_world.hpp)
        double *vel;          // [B][nworld][2] NED m/s
        double *trk_pv, *trk_lh; // [B][K][4], [B][K] the slot tracks a predicted prepare leaves between its two steps
        double *min_sep;      // [B] smallest distance to a vessel of the instance's scene (1e300 after a reset)
        int *sep_tick;        // [B] the prepare it was met at (-1: none yet)
        // exchanged plans (fleet_plan.hpp; usv_pf_fleet_plans / usv_guidance_fleet_plans), made when plans are first switched on
        int *chosen;          // [B][K] the list index behind each slot, as the last prepare's decide step chose
        int *source;          // [B][K] the vessel behind each plan-fed slot of the last prepare, -1: none
        unsigned long long *plan_fed; // [1] plan-fed (instance, slot) pairs so far
    } wb;
    long long plan_launches;  // launches of the plan kernel so far
    bool plan_source_clear;   // wb.source is all -1 (no memset is enqueued for a prepare that finds it so)
    int last_wide;            // the last RTI launch ran on the wide kernel
    // hand-over of long runners to a follow-up launch (option "handover_iter")
    int *d_susp_count, *d_susp_list; // [RING] instances each of the last launches handed over / [B] their groups
    double *d_susp_rec;       // [B][4] (DevPtrs::susp_rec)
    // the follow-up kernel beside the draining launch (usv_qp_resume_co; option "handover_co")
    bool co_ready;            // co_stream, ev_co_pre / ev_co_end and d_co_ctl exist (made together on first use: co_prepare)
    hipStream_t co_stream;
    hipEvent_t ev_co_pre, ev_co_end;
    int *d_co_ctl;            // [RING][8] DevPtrs::co_ctl of the last launches
    bool ev3_set[RING];       // ev[.][3] was recorded for that solve
    int ncu;                  // compute units of the device
    QpCaps caps;              // what the occupancy queries said about the QP kernels (qp_plan.hpp)
    bool map_changed;         // the group -> instance map differs from the one the workspace's multipliers were written under
    int *d_fail_ring;         // [RING] instances with status != 0, one slot per solve
    int *d_unconv_ring;       // [RING] instances whose QP did not converge to the tolerances (qp_status != 0), one slot per solve
    unsigned long long *d_unconv_total; // [1] ... summed over every RTI solve of the handle (usvmpc_unconverged_total)
    // Caller-visible arrays live in ONE device arena, in the order [x | u | status | x0 | yref | yref_e | p | lh] (256-byte aligned
    // pieces: field_plan.hpp, arena_layout).  Small handles also keep a pinned host MIRROR of it.  Which names a caller may set and get, where
    // the pieces lie, what the mirror holds newer than the device and whom it may answer is field_plan.hpp's: the field table and the state
    // machine HostMirror (no field of it is assigned in this file - copy_field, mirror_flush, launch_solve and the few callers that wait,
    // hand a pointer out or give the mirror up call its methods), host-only and checked on the CPU by tests/test_field_plan.py.  Here: the
    // two base pointers its offsets apply to.
    HostMirror hm;            // (hm.lay: the arena's layout)
    char *arena;              // device
    char *mirror;             // pinned host copy of the arena, or nullptr (hm.on false: arena larger than MIRROR_MAX, or given up)
    // Pipelined lineariser (option "pipeline_linearize"): the lineariser of tick t + 1 runs on a second stream beside the QP launch of tick t.
    // When, under which map and whether what it made still stands is lin_plan.hpp's: the state machine LinSched (no field of it is assigned
    // in this file - spec_cancel, copy_field, usvmpc_sync and launch_solve call its methods) and the per-solve plan plan_lin, both host-only
    // and checked on the CPU by tests/test_lin_plan.py.  Here: the HIP objects and the two map buffers the plan names.
    hipStream_t aux_stream;   // nullptr until first used
    hipEvent_t ev_pre, ev_spec;
    int *d_epoch, *d_redo, *d_perm2, *d_inv; // (d_perm / d_perm2: LinMap MAP_A / MAP_B)
    LinSched sched;
    long lin_pair_launches;   // launches of the paired kernels (option "lin_pairs") so far (usvmpc_lin_pair_launches)
    int *d_force_epoch, *d_force_redo, *d_force_inv; // option "lin_force_modes": epoch and redo words of a forced pair of launches, the running map's inverse
    // partial condensing (option "qp_cond_N")
    CondDims cond_dims;       // sizes of the condensed QP (valid when d_cond_dims is set)
    CondDims *d_cond_dims;
    double *d_cond_scratch;   // [cond_teams][cond_dims.total]
    long cond_teams;
    size_t cond_lds;          // dynamic LDS of the condensing kernel, bytes
    // Obstacle tracks (option "obstacle_tracks"): position and velocity per instance and obstacle slot, laid out like one stage of p.  While the
    // option is on p is DERIVED: every solve first runs usv_obstacle_predict on the main stream (launch_solve) - unless neither the tracks nor
    // the world clock nor the stages it writes changed since it last ran.  Buffers exist from the first set of a track field.
    double *d_obs_pos, *d_obs_vel;   // [B][2K] each
    double *d_clear, *d_clear_min;   // [B] clearance after the last world step / its minimum since the caller last set "obs_pos"
    bool tracks_pos_set;      // "obs_pos" has been set (or its device pointer handed out)
    bool tracks_dirty;        // p on the device is not what the tracks predict
    bool tracks_extern;       // a device pointer to a track field was handed out: the prediction runs before every solve
    bool clear_reset;         // the next world step starts the running minimum afresh (until then "clearance_min" reads 1e300)
    long export_at = -1;      // nsolves the multiplier read-back buffers (ptrs.lam_out / t_out) were filled at; -1: never
    bool last_cond;           // the last launch solved the partially condensed QP (its rows live in per-team scratch, not in the workspace)
    bool layout_dirty;        // the row layout option changed after the last solve: the workspace cannot be read back
    size_t bytes;
    std::string err;
    std::vector<void *> allocs;
    // The guidance front end's device-resident mode (usvmpc_guidance_world; the kernel: usv_guidance_tick): the world list lives on the device
    // and a prepare without host arrays reads the vessel's state from x0.  A moving world (usvmpc_guidance_world_vel) as the path-following
    // front end's: velocities per entry, every stage of p / lh written when it is predicted, moved on by usvmpc_advance / _advance_sim.
    CaTickPtrs gd_tickp = {};   // min_clear, finish_tick (the world, its tracks and tick: filled per launch)
    int gd_tick = 0;            // device-resident prepares since the last reset
    // Closed-loop log (usvmpc_log_*): which hand-over records, the counters and the layout are log_plan.hpp's - the state machine LogPlan (no
    // field of it is assigned in this file: usvmpc_log_start / _stop and log_handover call its methods), host-only and checked on the CPU by
    // tests/test_log_plan.py.  Here: the buffers its layout sizes (nullptr: channel not recorded) and the kernel arguments that do not change.
    LogPlan log;
    double *log_x = nullptr, *log_u = nullptr, *log_sums = nullptr; // [capacity][B][nsel], [capacity][B][nu], [2][B][n_err]
    int *log_status = nullptr;  // [capacity][B]
    LogRec log_rec = {};
    // Objective value (usvmpc_get "cost" .., usvmpc_eval_cost, usvmpc_cost_track): everything on first use - a handle that never asks for a
    // cost allocates nothing and launches what it always did.
    CostTab *d_cost_tab = nullptr;  // the kernels' tables (cost_eval.hpp)
    double *d_cost = nullptr, *d_cost_stage = nullptr, *d_cost_parts = nullptr; // [B], [B][N+1], [B][3]
    double *d_cost_sum = nullptr;   // [B] the realised closed-loop cost while tracking runs (nullptr: it does not)
    long long cost_count = 0;       // hand-overs that entered it
};

// Kernels::lin / lin_pair: usv_linearize for one and several RK4 steps (MULTI), every MODE
template <class M, int KCH, bool SOFT, bool PAIR, int... MODE>
void set_lin(group_kernel_t (&t)[2][LIN_MODES], std::integer_sequence<int, MODE...>)
{
    ((t[0][MODE] = &usv_linearize<M, KCH, SOFT, false, PAIR, MODE>, t[1][MODE] = &usv_linearize<M, KCH, SOFT, true, PAIR, MODE>), ...);
}

// The kernel table of one (model, obstacle chunks) pair for the handle's current row layout.  (External linkage: a split build defines
// each instantiation in a translation unit of its own - see "Build parts" at the top.)
template <class M, int KCH, bool SOFT>
Kernels kernels_for(const usvmpc_handle *h)
{
    constexpr bool CANPACK = KCH > 0;
    const DevSpec &S = h->spec;
    const bool pack = CANPACK && S.boxpack != 0;
    Kernels k = {};
    set_lin<M, KCH, SOFT, false>(k.lin, std::make_integer_sequence<int, LIN_MODES>{});
    if constexpr (PairCols<M>::ENABLED) set_lin<M, KCH, SOFT, true>(k.lin_pair, std::make_integer_sequence<int, LIN_MODES>{});
    k.qp_export = S.any_bsoft ? &usv_qp_export<M, KCH, SOFT, false, true>
                              : pack ? &usv_qp_export<M, KCH, SOFT, CANPACK, false> : &usv_qp_export<M, KCH, SOFT, false, false>;
    k.npt_hard = WsLayout<M, KCH, SOFT, false>::NPT; k.npt_soft = WsLayout<M, KCH, SOFT, true>::NPT;
    k.kch = KCH; k.soft = SOFT;
    auto qp = [&k](qp_kernel_t q, qp_kernel_t q_lds = nullptr, qp_kernel_t q_aux = nullptr) { k.qp[SLOT_QP] = q; k.qp[SLOT_QP_LDS] = q_lds; k.qp[SLOT_QP_AUX] = q_aux; };
    // (one row pass when every box row rides in a slot lane: qp_ipm.hpp, MERGE)
    const bool merge = pack && h->opt.merge_rows && !S.box_dense;
#ifdef USV_BENCH_ONLY // development builds (tools/dev_build.sh): only the instantiation the bench workload runs (k.qp[SLOT_QP] null for any other layout)
    if (!(S.hdiag && pack && !S.any_bsoft)) return k;
    if (merge) {
        qp(&usv_qp_rti<M, KCH, SOFT, true, CANPACK, false, false, CANPACK>, &usv_qp_rti<M, KCH, SOFT, true, CANPACK, false, true, CANPACK>,
           &usv_qp_rti<M, KCH, SOFT, true, CANPACK, false, false, CANPACK, true>);
        set_wide<M, KCH, SOFT, CANPACK>(k);
    } else {
        qp(&usv_qp_rti<M, KCH, SOFT, true, CANPACK, false>, &usv_qp_rti<M, KCH, SOFT, true, CANPACK, false, true>,
           &usv_qp_rti<M, KCH, SOFT, true, CANPACK, false, false, false, true>);
    }
#else
    if (S.any_bsoft) { // soft state bounds: rows with slacks, ten planes of their own
        if (S.hdiag) { qp(&usv_qp_rti<M, KCH, SOFT, true, false, true>); set_wide<M, KCH, SOFT, false, true>(k); }
        else qp(&usv_qp_rti<M, KCH, SOFT, false, false, true>);
    } else if (S.hdiag) { // (every OCP of the reference: the only instantiations that also come with the workspace in LDS)
        // (the packed layouts - every OCP of the reference, the bench workloads - also come with the aux plane in LDS)
        if (merge) {
            qp(&usv_qp_rti<M, KCH, SOFT, true, CANPACK, false, false, CANPACK>, &usv_qp_rti<M, KCH, SOFT, true, CANPACK, false, true, CANPACK>,
               &usv_qp_rti<M, KCH, SOFT, true, CANPACK, false, false, CANPACK, true>);
            set_wide<M, KCH, SOFT, CANPACK>(k);
        } else if (pack) {
            qp(&usv_qp_rti<M, KCH, SOFT, true, CANPACK, false>, &usv_qp_rti<M, KCH, SOFT, true, CANPACK, false, true>,
               &usv_qp_rti<M, KCH, SOFT, true, CANPACK, false, false, false, true>);
            set_wide<M, KCH, SOFT, false>(k);
        } else { // (box rows in planes of their own)
            qp(&usv_qp_rti<M, KCH, SOFT, true, false, false>, &usv_qp_rti<M, KCH, SOFT, true, false, false, true>);
            set_wide<M, KCH, SOFT, false, false, true>(k);
        }
    } else {
        qp(pack ? &usv_qp_rti<M, KCH, SOFT, false, CANPACK, false> : &usv_qp_rti<M, KCH, SOFT, false, false, false>);
    }
#endif
    return k;
}

// The instantiations of the stock library: USV_KERNELS(PART, ...) names the pair build part PART compiles; every part declares all of them
// (extern template) and part PART then defines its own.
template <int PART> struct PartPair;
#define USV_KERNELS(PART, M, KCH, SOFT)                                                              \
    template <> struct PartPair<PART> { using Model = M; static constexpr int kch = KCH; static constexpr bool soft = SOFT; }; \
    extern template Kernels kernels_for<M, KCH, SOFT>(const usvmpc_handle *);
#if USV_PART >= 0 && !defined(USV_GEN_ONLY)
USV_KERNELS(1, ModelM0, 0, false)
USV_KERNELS(2, ModelM1, 1, true)
USV_KERNELS(3, ModelM1, 2, true)
USV_KERNELS(4, ModelM2, 1, false)
USV_KERNELS(5, ModelM2, 2, false)
#if USV_PART > 0
template Kernels kernels_for<PartPair<USV_PART>::Model, PartPair<USV_PART>::kch, PartPair<USV_PART>::soft>(const usvmpc_handle *);
#endif
#endif

#if USV_MAIN
// A kernel's dynamic-LDS limit belongs to the process, not to a handle: it is kept at the largest size any handle has launched the kernel
// with (a handle with a shorter horizon created later must not lower it under what an older one uses)
hipError_t usv::set_dynamic_lds(const void *kern, size_t bytes)
{
    static std::mutex mu;
    static std::unordered_map<const void *, size_t> largest;
    std::lock_guard<std::mutex> lock(mu);
    size_t &cur = largest[kern];
    if (bytes <= cur) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) cur = bytes;
    return e;
}

namespace {

thread_local std::string g_create_err;

#define HIP_TRY(h, call)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                         \
            return USVMPC_E_HIP;                                                                  \
        }                                                                                         \
    } while (0)

template <class T>
int dev_alloc(usvmpc_handle *h, T **p, size_t count, bool zero)
{
    const size_t nbytes = (count ? count : 1) * sizeof(T);
    HIP_TRY(h, hipMalloc((void **)p, nbytes));
    h->allocs.push_back((void *)*p);
    h->bytes += nbytes;
    // on the handle's stream: it is non-blocking, i.e. NOT ordered against the legacy default stream hipMemset uses
    if (zero) HIP_TRY(h, hipMemsetAsync((void *)*p, 0, nbytes, h->stream));
    return 0;
}

// release one buffer obtained from dev_alloc (growing a guidance buffer replaces it)
void dev_free(usvmpc_handle *h, void *p, size_t nbytes)
{
    if (!p) return;
    for (size_t i = 0; i < h->allocs.size(); i++)
        if (h->allocs[i] == p) { h->allocs.erase(h->allocs.begin() + (long)i); break; }
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(p);
    h->bytes -= nbytes;
}

// the device array behind a row of the field table (field_plan.hpp): the only place where names meet pointers
void *field_ptr(usvmpc_handle *h, FieldId id)
{
    const DevPtrs &P = h->ptrs;
    const void *const by_id[] = {P.x, P.u, P.status, P.x0, P.yref, P.yref_e, P.p, P.lh, // (in FieldId's order)
                                 P.pi, P.sl, P.su, P.res, P.obs_tmin, P.nlp_res, P.lam_out, P.t_out, P.qp_iter, P.qp_status, P.sqp_iter,
                                 h->d_obs_pos, h->d_obs_vel, h->d_clear, h->d_clear_min, h->d_cost, h->d_cost_stage, h->d_cost_parts};
    static_assert(sizeof by_id / sizeof *by_id == FLD_COUNT && FLD_PI == 8 && FLD_QP_ITER == 16 && FLD_OBS_POS == 19 && FLD_COST == 23,
                  "one pointer per row of the field table");
    return const_cast<void *>(by_id[id]);
}

static_assert(FIELD_E_UNKNOWN == USVMPC_E_FIELD, "field_plan.hpp restates the code");
FieldDims field_dims(const usvmpc_handle *h)
{
    return FieldDims{h->N, h->nx, h->nu, h->ny, h->ny_e, h->K, h->ptrs.nlam, h->ptrs.lam_out && h->ptrs.t_out};
}

int ensure_export(usvmpc_handle *h); // (below: needs the kernel dispatch)

// the speculative lineariser of the second stream: wait for it and forget what it made (something it read or wrote is about to change)
int spec_cancel(usvmpc_handle *h)
{
    if (h->sched.cancel()) {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipStreamSynchronize(h->aux_stream));
    }
    return 0;
}

// wait for a mirror <-> arena copy that may still be running before the host touches the mirror
int mirror_quiesce(usvmpc_handle *h)
{
    if (h->hm.must_wait()) {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->hm.synced();
    }
    return 0;
}

// the executor of a copy descriptor (field_plan.hpp), on the handle's stream: c.rows pieces of c.width bytes between device memory (pieces
// c.pitch apart) and host memory (host_pitch apart), up or down
int exec_copy(usvmpc_handle *h, char *dev, char *host, size_t host_pitch, const CopyDesc &c, bool up)
{
    const hipMemcpyKind kind = up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    if (c.rows == 1) HIP_TRY(h, hipMemcpyAsync(up ? dev : host, up ? host : dev, c.width, kind, h->stream));
    else HIP_TRY(h, hipMemcpy2DAsync(up ? dev : host, up ? c.pitch : host_pitch, up ? host : dev, up ? host_pitch : c.pitch, c.width, c.rows, kind, h->stream));
    return 0;
}
// ... between the arena and its mirror: the same bytes of both
int mirror_copy(usvmpc_handle *h, const CopyDesc &c, bool up) { return exec_copy(h, h->arena + c.off, h->mirror + c.off, c.pitch, c, up); }

// upload what the mirror holds newer than the device (HostMirror::next_upload: runs of dirty stages, consecutive dirty fields as one copy)
int mirror_flush(usvmpc_handle *h)
{
    CopyDesc c;
    while (h->hm.next_upload(c)) {
        const int rc = mirror_copy(h, c, true);
        if (rc) return rc;
    }
    return 0;
}

// ---- obstacle tracks (usvmpc_handle: d_obs_pos ..): buffers on first use, the caller-visible fields, the two launches
int tracks_alloc(usvmpc_handle *h)
{
    if (h->K == 0) { h->err = "obstacle tracks: this model has no obstacle rows (K = 0)"; return USVMPC_E_FIELD; }
    if (h->d_obs_pos) return 0;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t B = (size_t)h->B, n = B * 2 * (size_t)h->K;
    double *pos = nullptr, *vel = nullptr, *cl = nullptr, *clm = nullptr;
    if (dev_alloc(h, &pos, n, true) || dev_alloc(h, &vel, n, true) || dev_alloc(h, &cl, B, false) || dev_alloc(h, &clm, B, false))
        return USVMPC_E_HIP;
    const std::vector<double> far(B, 1e300); // (no world step yet)
    HIP_TRY(h, hipMemcpyAsync(cl, far.data(), B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(clm, far.data(), B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->d_obs_pos = pos; h->d_obs_vel = vel; h->d_clear = cl; h->d_clear_min = clm;
    return 0;
}

// usvmpc_set / usvmpc_get of "obs_pos" / "obs_vel" ([B][2K]) and usvmpc_get of "clearance" / "clearance_min" ([B]); the stage is ignored
int tracks_field(usvmpc_handle *h, const std::string &s, double *host, size_t n, bool set)
{
    if (h->K == 0) { h->err = "field '" + s + "': this model has no obstacle rows (K = 0), hence no obstacle tracks"; return USVMPC_E_FIELD; }
    const bool track = s == "obs_pos" || s == "obs_vel";
    if (set && !track) { h->err = "field '" + s + "' is read-only"; return USVMPC_E_FIELD; }
    const size_t want = track ? 2 * (size_t)h->K : 1;
    if (n != want) {
        h->err = "mismatching dimension for field '" + s + "': expected " + std::to_string(want) + ", got " + std::to_string(n);
        return USVMPC_E_SIZE;
    }
    if (!set && !h->d_obs_pos) { h->err = "field '" + s + "': no obstacle tracks yet (set \"obs_pos\" first)"; return USVMPC_E_ARG; }
    const int rca = tracks_alloc(h);
    if (rca) return rca;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nbytes = (size_t)h->B * want * sizeof(double);
    if (set) {
        HIP_TRY(h, hipMemcpyAsync(s == "obs_pos" ? h->d_obs_pos : h->d_obs_vel, host, nbytes, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->tracks_dirty = true;
        if (s == "obs_pos") { h->tracks_pos_set = true; h->clear_reset = true; }
        return 0;
    }
    if (s == "clearance_min" && h->clear_reset) { // (the positions were set anew and the world has not moved since)
        for (int b = 0; b < h->B; b++) host[b] = 1e300;
        return 0;
    }
    const double *src = s == "obs_pos" ? h->d_obs_pos : s == "obs_vel" ? h->d_obs_vel : s == "clearance" ? h->d_clear : h->d_clear_min;
    HIP_TRY(h, hipMemcpyAsync(host, src, nbytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

// position states of the handle's model (the states its obstacle rows read)
bool model_pos_index(int model, int &ipx, int &ipy)
{
    switch (model) {
#ifndef USV_GEN_ONLY
    case USVMPC_MODEL_GUIDANCE_CA1: ipx = ModelM1::IPX; ipy = ModelM1::IPY; return true;
    case USVMPC_MODEL_PF_CA: ipx = ModelM2::IPX; ipy = ModelM2::IPY; return true;
#endif
#ifdef USV_GEN_MODEL_HEADER
    case USVMPC_MODEL_GENERATED: ipx = ModelGen::IPX; ipy = ModelGen::IPY; return true;
#endif
    }
    return false;
}

// p <- the tracks' prediction, on the main stream (launch_solve: behind the upload of pending host writes, ahead of every reader of p)
int tracks_predict(usvmpc_handle *h)
{
    const int last = h->spec.p_static ? 0 : h->N;
    hipLaunchKernelGGL(usv_obstacle_predict, dim3((unsigned)h->B), dim3(256), 0, h->stream, (const double2 *)h->d_obs_pos,
                       (const double2 *)h->d_obs_vel, (double2 *)const_cast<double *>(h->ptrs.p), h->N, h->K, last, h->spec.dt);
    HIP_TRY(h, hipGetLastError());
    h->tracks_dirty = false;
    return 0;
}

// the world step (usvmpc_obstacles_step; usvmpc_advance / _advance_sim behind their own kernel): enqueued on the main stream
int tracks_step(usvmpc_handle *h, double T)
{
    if (!h->d_obs_pos || !h->tracks_pos_set) { h->err = "obstacles_step: no obstacle tracks yet (set \"obs_pos\" first)"; return USVMPC_E_ARG; }
    if (!(T == T) || T - T != 0.0) { h->err = "obstacles_step: T must be finite"; return USVMPC_E_ARG; }
    int ipx = 0, ipy = 0;
    if (!model_pos_index(h->desc.model, ipx, ipy)) { h->err = "obstacles_step: this model has no position states"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    {   // (x0 and lh are read: pending host writes go up first)
        const int rcf = mirror_flush(h);
        if (rcf) return rcf;
    }
    hipLaunchKernelGGL(usv_obstacle_step, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, h->stream, h->d_obs_pos, (const double *)h->d_obs_vel,
                       h->ptrs.x0, h->ptrs.lh, h->d_clear, h->d_clear_min, h->B, h->K, h->N, h->nx, ipx, ipy, T, h->clear_reset ? 1 : 0);
    HIP_TRY(h, hipGetLastError());
    h->clear_reset = false;
    h->tracks_dirty = true;
    return 0;
}

// ---- objective value (usvmpc_handle: d_cost_tab ..): what every entry point refuses, the buffers on first use, the two launches
int cost_check(usvmpc_handle *h)
{
    // (the slack values of soft state bounds are not among the arrays a caller can get: their share of the cost could not be restated)
    if (h->spec.any_bsoft) { h->err = "cost: not built for soft state bounds"; return USVMPC_E_ARG; }
    return 0;
}

int cost_tab_ensure(usvmpc_handle *h)
{
    if (h->d_cost_tab) return 0;
    HIP_TRY(h, hipSetDevice(h->device));
    const usvmpc_desc &d = h->desc;
    CostTab T;
    cost_fill_tab(T, h->nx, h->nu, h->ny, h->ny_e, h->soft ? h->K : 0, d.Vu, d.Vx, d.W, d.Vx_e, d.W_e, d.zl, d.zu, d.Zl, d.Zu);
    CostTab *tab = nullptr;
    if (dev_alloc(h, &tab, 1, false)) return USVMPC_E_HIP;
    HIP_TRY(h, hipMemcpyAsync(tab, &T, sizeof(CostTab), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // (T is a local)
    h->d_cost_tab = tab;
    return 0;
}

int cost_alloc(usvmpc_handle *h)
{
    if (h->d_cost) return 0;
    const int rct = cost_tab_ensure(h);
    if (rct) return rct;
    const size_t B = (size_t)h->B;
    double *c = nullptr, *cs = nullptr, *cp = nullptr;
    if (dev_alloc(h, &c, B, true) || dev_alloc(h, &cs, B * (size_t)(h->N + 1), true) || dev_alloc(h, &cp, B * 3, true)) return USVMPC_E_HIP;
    h->d_cost = c; h->d_cost_stage = cs; h->d_cost_parts = cp;
    return 0;
}

CostArgs cost_args(const usvmpc_handle *h)
{
    CostArgs a = {};
    const DevPtrs &P = h->ptrs;
    a.tab = h->d_cost_tab;
    a.x = P.x; a.u = P.u; a.yref = P.yref; a.yref_e = P.yref_e; a.sl = P.sl; a.su = P.su; a.x0 = P.x0;
    a.cost_stage = h->d_cost_stage; a.cost = h->d_cost; a.parts = h->d_cost_parts; a.sum = h->d_cost_sum;
    a.B = h->B; a.N = h->N; a.nx = h->nx; a.nu = h->nu; a.ny = h->ny; a.ny_e = h->ny_e;
    a.K = h->K; a.Ks = h->soft ? h->K : 0;
    a.dt = h->spec.dt;
    return a;
}

// usv_cost_eval enqueued on the main stream, behind the upload of pending host writes (it reads x, u, yref).  No caller write: it writes cost
// memory only, so the pipelined lineariser's pass made a tick ahead stands (as for usv_log_record).
int cost_enqueue(usvmpc_handle *h)
{
    int rc = cost_check(h);
    if (rc) return rc;
    rc = cost_alloc(h);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = mirror_flush(h);
    if (rc) return rc;
    hipLaunchKernelGGL(h->soft && h->K > 0 ? usv_cost_eval<true> : usv_cost_eval<false>, dim3((unsigned)((h->B + 3) / 4)), dim3(256), 0, h->stream, cost_args(h));
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// a hand-over of a handle that tracks its realised cost (usvmpc_advance / usvmpc_advance_sim, behind the mirror's upload and ahead of their own kernel)
int cost_handover(usvmpc_handle *h)
{
    hipLaunchKernelGGL(h->soft && h->K > 0 ? usv_cost_track<true> : usv_cost_track<false>, dim3((unsigned)((h->B + 16 * COST_TRACK_EACH - 1) / (16 * COST_TRACK_EACH))), dim3(256), 0,
                       h->stream, cost_args(h));
    HIP_TRY(h, hipGetLastError());
    h->cost_count++;
    return 0;
}

// usvmpc_set / usvmpc_get: the name resolved through the field table, validated once, then either a memcpy into / out of the pinned mirror
// (HostMirror says whether, and what that leaves to upload) or one copy to / from the device, synchronised
int copy_field(usvmpc_handle *h, const char *field, int stage, double *host, size_t n, bool set)
{
    if (!h) return USVMPC_E_ARG;
    const FieldRow *row = find_field(field);
    const unsigned flags = row ? row->flags : 0;
    if ((flags & FF_TRACK) && h->K == 0) return tracks_field(h, field, host, n, set); // (the field error, whatever the buffer)
    if (!host) { h->err = "null buffer"; return USVMPC_E_ARG; }
    if (flags & FF_TRACK) return tracks_field(h, field, host, n, set);
    if (set && h->opt.tracks_on && row && row->id == FLD_P) {
        h->err = "field 'p' is derived from the obstacle tracks while option \"obstacle_tracks\" is 1: set \"obs_pos\" / \"obs_vel\", or switch the option off";
        return USVMPC_E_ARG;
    }
    if (!set && (flags & FF_EXPORT)) {
        const int rce = ensure_export(h);
        if (rce) return rce;
    }
    if (!set && (flags & FF_COST)) {
        const int rcc = cost_check(h);
        if (rcc) return rcc;
    }
    Field f;
    if (resolve(row, stage, field_dims(h), set, f)) {
        h->err = std::string("unknown field '") + (field ? field : "") + "'";
        return USVMPC_E_FIELD;
    }
    if (set && (f.row->flags & FF_PF)) h->pf_stale = true; // (the path-following front end rewrites its rows)
    if ((int)n != f.n) {
        h->err = std::string("mismatching dimension for field '") + field + "': expected " + std::to_string(f.n) +
                 ", got " + std::to_string(n);
        return USVMPC_E_SIZE;
    }
    if (f.n == 0) return 0;
    if (const int bad = stage_check(f)) {
        h->err = bad == 1 ? std::string("stage ") + std::to_string(f.stage) + " out of range for field '" + field + "'" : std::string("stage out of range");
        return USVMPC_E_STAGE;
    }
    // (a lineariser that ran ahead may have read what is being replaced - it reads x, u, yref: the next solve linearises again)
    if (set && (f.row->flags & FF_LIN)) h->sched.caller_wrote();
    if (set && f.row->id == FLD_X) h->world.plan_lost(); // (exchanged plans: the iterate is the caller's now)
    const CopyDesc span = field_span(f, (size_t)h->B);
    const int slot = f.row->slot;
    if (set ? h->hm.set_served(slot) : h->hm.get_served(slot)) {
        // ---- through the pinned mirror: no HIP call unless a copy is still in flight
        const int rc = mirror_quiesce(h);
        if (rc) return rc;
        char *m = h->mirror + h->hm.lay.off[slot] + span.off;
        for (size_t b = 0; b < span.rows; b++) {
            if (set) std::memcpy(m + b * span.pitch, (const char *)host + b * span.width, span.width);
            else std::memcpy((char *)host + b * span.width, m + b * span.pitch, span.width);
        }
        CopyDesc now;
        if (set && h->hm.wrote(slot, span, now)) { // (a strided stage under a handed-out device pointer goes up at once)
            HIP_TRY(h, hipSetDevice(h->device));
            return mirror_copy(h, now, true);
        }
        return 0;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    if (!set) { // (a get of a field with pending writes sees them)
        const int rc = mirror_flush(h);
        if (rc) return rc;
    }
    if (!set && (f.row->flags & FF_COST)) { // (an objective value: evaluated now, of the iterate the device holds; no staleness state is kept)
        const int rc = cost_enqueue(h);
        if (rc) return rc;
    }
    const int rc = exec_copy(h, (char *)field_ptr(h, f.row->id) + span.off, (char *)host, span.width, span, set);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->hm.synced();
    return 0;
}

// the condensed QP solve of an RTI iteration (after the lineariser): buffers on first use; the kernels live in cond_kernels.hip
int launch_cond(usvmpc_handle *h)
{
    if (!h->d_cond_dims) {
        CondDims D;
        size_t lds = 0;
        int nb = 0;
        const int rcp = cond_prepare(h->desc.model, h->kch, h->spec, h->opt.cond_N2, D, lds, nb, h->err);
        if (rcp) return rcp;
        if (nb < 1 || h->ncu < 1) { h->err = "partial condensing: the kernel cannot be launched with this much LDS"; return USVMPC_E_HIP; }
        long teams = std::min<long>(h->B, (long)nb * h->ncu);
        if (h->opt.max_waves > 0) teams = std::min<long>(teams, h->opt.max_waves);
        if (dev_alloc(h, &h->d_cond_dims, 1, false)) return USVMPC_E_HIP;
        if (dev_alloc(h, &h->d_cond_scratch, (size_t)teams * (size_t)D.total, true)) return USVMPC_E_HIP;
        HIP_TRY(h, hipMemcpyAsync(h->d_cond_dims, &D, sizeof(CondDims), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream)); // (D is a local)
        h->cond_dims = D; h->cond_teams = teams; h->cond_lds = lds;
    }
    HIP_TRY(h, hipMemsetAsync(h->ptrs.queue, 0, sizeof(int), h->stream));
    if (h->ptrs.lam_out) { // multiplier read-back: this solve fills the buffers (rows a stage does not have read 0)
        const size_t nbytes = (size_t)h->B * (h->N + 1) * (size_t)(h->ptrs.nlam > 0 ? h->ptrs.nlam : 1) * sizeof(double);
        HIP_TRY(h, hipMemsetAsync(h->ptrs.lam_out, 0, nbytes, h->stream));
        HIP_TRY(h, hipMemsetAsync(h->ptrs.t_out, 0, nbytes, h->stream));
        h->export_at = h->nsolves + 1;
    }
    const int rcr = cond_run(h->desc.model, h->kch, h->cond_dims, h->stream, h->cond_teams, h->cond_lds, h->ptrs, h->d_cond_dims, h->d_cond_scratch, h->B, h->err);
    if (rcr) return rcr;
    h->map_changed = true; // (the group-indexed workspace holds no multipliers of this QP: a later full SQP starts afresh)
    return 0;
}

void cond_release(usvmpc_handle *h)
{
    if (h->d_cond_scratch) dev_free(h, h->d_cond_scratch, (size_t)h->cond_teams * (size_t)h->cond_dims.total * sizeof(double));
    if (h->d_cond_dims) dev_free(h, h->d_cond_dims, sizeof(CondDims));
    h->d_cond_scratch = nullptr; h->d_cond_dims = nullptr; h->cond_teams = 0;
}

// Workgroups of `block` threads a CU holds of `kern` with `dyn` bytes of dynamic LDS (the kernel's limit raised to that first); 0: it does
// not fit - static and dynamic LDS over a CU's 160 KB - or a call failed
int blocks_per_cu(const void *f, int block, size_t dyn)
{
    hipFuncAttributes fa;
    int nb = 0;
    if (f == nullptr || hipFuncGetAttributes(&fa, f) != hipSuccess || fa.sharedSizeBytes + dyn > (size_t)CU_LDS_BYTES || set_dynamic_lds(f, dyn) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, block, dyn) != hipSuccess)
        return 0;
    return nb;
}

// The co-resident follow-up kernel's stream, events and control ring: made together on first use, co_ready set last.  When one of them
// cannot be made, what was made is released and the handle's hand-overs go to the follow-up launch behind the main one only.
void co_release(usvmpc_handle *h)
{
    if (h->co_stream) { (void)hipStreamSynchronize(h->co_stream); (void)hipStreamDestroy(h->co_stream); }
    if (h->ev_co_pre) (void)hipEventDestroy(h->ev_co_pre);
    if (h->ev_co_end) (void)hipEventDestroy(h->ev_co_end);
    dev_free(h, h->d_co_ctl, (size_t)usvmpc_handle::RING * 8 * sizeof(int));
    h->co_stream = nullptr; h->ev_co_pre = nullptr; h->ev_co_end = nullptr; h->d_co_ctl = nullptr;
    h->co_ready = false;
}

bool co_prepare(usvmpc_handle *h)
{
    if (h->co_ready) return true;
    int prio_least = 0, prio_greatest = 0;
    const bool ok = hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) == hipSuccess &&
                    hipStreamCreateWithPriority(&h->co_stream, hipStreamNonBlocking, prio_least) == hipSuccess &&
                    hipEventCreateWithFlags(&h->ev_co_pre, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&h->ev_co_end, hipEventDisableTiming) == hipSuccess &&
                    dev_alloc(h, &h->d_co_ctl, (size_t)usvmpc_handle::RING * 8, true) == 0;
    if (ok) h->co_ready = true;
    else { co_release(h); h->opt.handover_co = 0; (void)hipGetLastError(); } // (handled here: the launch's own error check must not report it)
    return ok;
}

// The QP launches of an RTI solve or of one iteration of the full SQP, as qp_plan.hpp's plan_qp lays them out for the handle's sizes, options and kernel table (every threshold of
// the mapping lives there, with the measurement behind it); here: the occupancy queries it asks, the buffers of a first hand-over, the
// launches.
int launch_qp(usvmpc_handle *h, const Kernels &k, int phase)
{
    static_assert(QP_GROUP_LANES == LANES, "qp_plan.hpp sizes the grid of the throughput mapping");
    QpIn in = {};
    in.B = h->B; in.Bp = h->Bp; in.N = h->N; in.K = h->K;
    in.npt = h->spec.npt; in.nu = h->nu; in.aux_dense4 = h->spec.aux_dense4; in.kch = h->kch; in.phase = phase; in.ncu = h->ncu;
    in.wide_mode = h->opt.wide_mode; in.wide_waves = h->opt.wide_waves; in.lds_mode = h->opt.lds_mode; in.dynamic_rows = h->opt.dynamic_rows;
    in.max_waves = h->opt.max_waves; in.aux_lds = h->opt.aux_lds; in.handover_iter = h->opt.handover_iter; in.handover_lds = h->opt.handover_lds;
    in.handover_co = h->opt.handover_co; in.co_wgs = h->opt.co_wgs; in.own_stream = h->own_stream;
    for (int s = 0; s < SLOT_QP_KERNELS; s++) in.has[s] = k.qp[s] != nullptr;
    in.has[SLOT_RESUME] = k.resume != nullptr; in.has[SLOT_RESUME_LDS] = k.resume_lds != nullptr; in.has_resume_co = k.resume_co != nullptr;
    in.nplw = k.nplw; in.ex_lds = k.ex_lds; in.ex_hbm = k.ex_hbm; in.k_kch = k.kch; in.k_soft = k.soft;
    struct {
        const Kernels &k;
        const void *kernel(QpSlot s) const
        {
            return s < SLOT_QP_KERNELS ? (const void *)k.qp[s] : s == SLOT_RESUME ? (const void *)k.resume : (const void *)k.resume_lds;
        }
        int blocks(QpSlot s, int block, size_t dyn) const { return blocks_per_cu(kernel(s), block, dyn); }
        long static_lds(QpSlot s) const
        {
            hipFuncAttributes fa;
            return hipFuncGetAttributes(&fa, kernel(s)) == hipSuccess ? (long)fa.sharedSizeBytes : 0;
        }
    } probe = {k};
    const QpPlan p = plan_qp(in, h->caps, probe);
    const int slot_now = (int)(h->nsolves % usvmpc_handle::RING);
    hipEvent_t *ev = h->ev[slot_now];
    h->last_wide = p.mapping;
    h->ptrs.susp_count = nullptr; h->ptrs.susp_list = nullptr; h->ptrs.susp_rec = nullptr; h->ptrs.handover_iter = 0; h->ptrs.co_ctl = nullptr; // (set below when the launch hands over)
    if (p.q0 >= 0) HIP_TRY(h, hipMemsetAsync(h->ptrs.queue, 0, sizeof(int), h->stream));
    if (p.hand_ready && !h->d_susp_list) {
        if (dev_alloc(h, &h->d_susp_count, (size_t)usvmpc_handle::RING, true) || dev_alloc(h, &h->d_susp_list, (size_t)h->B, false) ||
            dev_alloc(h, &h->d_susp_rec, (size_t)h->B * 4, false))
            return USVMPC_E_HIP;
    }
    if (p.hand) {
        h->ptrs.susp_count = h->d_susp_count + slot_now;
        h->ptrs.susp_list = h->d_susp_list;
        h->ptrs.susp_rec = h->d_susp_rec;
        h->ptrs.handover_iter = p.hand_iter;
    }
    // (when its stream cannot be made the option goes off for the handle and the launch goes on without it: co_prepare)
    const bool co = p.co && co_prepare(h);
    if (co) {
        HIP_TRY(h, set_dynamic_lds((const void *)k.resume_co, p.hand_bytes));
        h->ptrs.co_ctl = h->d_co_ctl + 8 * slot_now;
        HIP_TRY(h, hipMemsetAsync(h->ptrs.co_ctl, 0, 8 * sizeof(int), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->d_susp_list, 0xff, (size_t)h->B * sizeof(int), h->stream)); // (-1: no entry yet)
        HIP_TRY(h, hipEventRecord(h->ev_co_pre, h->stream));
    }
    hipLaunchKernelGGL(k.qp[p.slot], dim3((unsigned)p.grid), dim3(p.block), p.lds_bytes, h->stream, h->ptrs, p.ngroups, phase, p.q0, p.rows);
    if (co) {
        hipLaunchKernelGGL(usv_co_done, dim3(1), dim3(1), 0, h->stream, h->ptrs.co_ctl);
        HIP_TRY(h, hipStreamWaitEvent(h->co_stream, h->ev_co_pre, 0));
        hipLaunchKernelGGL(k.resume_co, dim3((unsigned)p.co_wgs), dim3(QP_BLOCK), p.hand_bytes, h->co_stream, h->ptrs, (int)p.grid, (int)h->B, h->opt.co_spin_limit);
        HIP_TRY(h, hipEventRecord(h->ev_co_end, h->co_stream));
    }
    if (p.hand) {
        HIP_TRY(h, hipEventRecord(ev[3], h->stream));
        h->ev3_set[slot_now] = true;
        hipLaunchKernelGGL(p.hand_lds ? k.resume_lds : k.resume, dim3((unsigned)p.hand_wgs), dim3(QP_BLOCK), p.hand_bytes, h->stream, h->ptrs);
    }
    if (co) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_co_end, 0)); // (the tick's QPs are solved when both kernels are through)
    return 0;
}

// counting sort of the previous solve's iteration counts into a group -> instance map
int sort_into(usvmpc_handle *h, int *dst, int *inv)
{
    const int B = h->B;
    const int *prev2 = h->opt.sort_two ? h->d_iter_prev : h->ptrs.qp_iter; // (option "sort_two_ticks" = 0: the last count alone)
    hipLaunchKernelGGL(usv_sort_hist, dim3((B + 255) / 256), dim3(256), 0, h->stream, h->ptrs.qp_iter, prev2, B, h->d_hist);
    hipLaunchKernelGGL(usv_sort_scan, dim3(1), dim3(64), 0, h->stream, h->d_hist, h->d_cursor);
    hipLaunchKernelGGL(usv_sort_scatter, dim3((B + 255) / 256), dim3(256), 0, h->stream, h->ptrs.qp_iter, prev2, B, h->d_cursor, dst, inv);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// The pipelined lineariser's stream (lowest priority: lin_plan.hpp says why), events and buffers, made together on first use
int pipe_prepare(usvmpc_handle *h)
{
    const size_t B = (size_t)h->B;
    int prio_least = 0, prio_greatest = 0;
    HIP_TRY(h, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    HIP_TRY(h, hipStreamCreateWithPriority(&h->aux_stream, hipStreamNonBlocking, prio_least));
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_pre, hipEventDisableTiming));
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_spec, hipEventDisableTiming));
    if (dev_alloc(h, &h->d_epoch, B, false) || dev_alloc(h, &h->d_redo, B * redo_words(h->N), true) ||
        dev_alloc(h, &h->d_perm2, B, true) || dev_alloc(h, &h->d_inv, B, true))
        return USVMPC_E_HIP;
    HIP_TRY(h, hipMemsetAsync(h->d_epoch, 0xff, B * sizeof(int), h->stream)); // -1: nothing is final yet
    return 0;
}

// Option "lin_force_modes" (Options::lin_force): the arguments of a forced pair of launches - epoch and redo words of their own, filled
// here, and the inverse of the running map
int force_prepare(usvmpc_handle *h, int epoch, DevPtrs &Pf)
{
    const int B = h->B;
    const size_t nredo = (size_t)B * h->ptrs.redo_words;
    if (!h->d_force_epoch && (dev_alloc(h, &h->d_force_epoch, (size_t)B, false) || dev_alloc(h, &h->d_force_redo, nredo, false) ||
                              dev_alloc(h, &h->d_force_inv, (size_t)B, false)))
        return USVMPC_E_HIP;
    Pf = h->ptrs;
    Pf.epoch = h->d_force_epoch;
    Pf.redo = h->d_force_redo;
    HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)h->d_force_epoch, epoch, (size_t)B, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_force_redo, 0, nredo * sizeof(int), h->stream));
    if (Pf.perm) {
        hipLaunchKernelGGL(usv_invert_map, dim3((B + 255) / 256), dim3(256), 0, h->stream, Pf.perm, B, h->d_force_inv);
        Pf.inv_next = h->d_force_inv;
    }
    return 0;
}

// One solve's launches on the handle's stream: sort, lineariser, the QP (launch_qp, or the partially condensed QP: launch_cond), the count
// of unconverged QPs and the copy of the results into the host mirror.  What the lineariser does, under which map and whether the next
// tick's runs ahead is lin_plan.hpp's plan_lin over the handle's LinSched: this function fills LinIn and carries the plan out.
int launch_solve(usvmpc_handle *h, const Kernels &k, int phase)
{
    static_assert(LIN_GROUP_LANES == LANES, "lin_plan.hpp sizes the lineariser's grids");
    {   // pending host writes go up first; the results come back below
        const int rcf = mirror_flush(h);
        if (rcf) return rcf;
    }
    // option "obstacle_tracks": p is what the tracks predict (the lineariser - the pipelined one included - never reads p: nothing made ahead
    // of time is invalidated; skipped while tracks, world clock and the stages written are what they were - not under a caller's device pointer)
    if (h->opt.tracks_on && (h->tracks_dirty || h->tracks_extern)) {
        const int rct = tracks_predict(h);
        if (rct) return rct;
    }
    const bool pairs = h->opt.lin_pairs != 0;
    if (pairs && k.lin_pair[0][0] == nullptr) { h->err = "lin_pairs: the model does not declare the columns to integrate"; return USVMPC_E_ARG; }
    const group_kernel_t *lin = (pairs ? k.lin_pair : k.lin)[h->spec.sim_steps > 1 ? 1 : 0]; // [MODE]
    const bool cond = phase == 0 && h->opt.cond_N2 > 0; // RTI solve on the partially condensed QP (cond_ipm.hpp)
    const int B = h->B;
    const int slot = (int)(h->nsolves % usvmpc_handle::RING); // this solve's place in the per-solve rings
    hipEvent_t *ev = h->ev[slot];
    auto map_buf = [h](LinMap m) { return m == MAP_A ? h->d_perm : m == MAP_B ? h->d_perm2 : nullptr; };
    LinIn in = {};
    in.phase = phase; in.nsolves = h->nsolves; in.B = B; in.Bp = h->Bp; in.N = h->N;
    in.pipeline = h->opt.pipeline; in.dynamic_rows = h->opt.dynamic_rows; in.sort_enabled = h->opt.sort_enabled; in.sort_two = h->opt.sort_two;
    in.lin_force = h->opt.lin_force; in.pairs = pairs; in.cond = h->opt.cond_N2 > 0;
    in.mirror = h->hm.on; in.extern_access = h->hm.extern_access;
    in.cur_map = !h->ptrs.perm ? MAP_NONE : h->ptrs.perm == h->d_perm ? MAP_A : MAP_B;
    const LinPlan p = plan_lin(in, h->sched);
    if (p.pipe && !h->aux_stream) {
        const int rcp = pipe_prepare(h);
        if (rcp) return rcp;
    }
    if (p.wait_ahead) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_spec, 0));
    if (p.map_changed) h->map_changed = true;
    if (p.map_from == LinPlan::SORT && sort_into(h, map_buf(p.map), nullptr)) return USVMPC_E_HIP;
    if (p.map_from != LinPlan::KEEP) h->ptrs.perm = map_buf(p.map);
    h->ptrs.epoch = p.spec_next ? h->d_epoch : nullptr;
    h->ptrs.redo = p.redo ? h->d_redo : nullptr;
    h->ptrs.redo_words = redo_words(h->N);
    h->ptrs.perm_cur = nullptr;
    h->ptrs.inv_next = nullptr;
    h->ptrs.tick = (int)h->nsolves;
    h->ev3_set[slot] = false;
    HIP_TRY(h, hipEventRecord(ev[0], h->stream));
    const DevPtrs *Pl = &h->ptrs;
    DevPtrs Pf;
    if (p.forced) {
        const int rcf = force_prepare(h, p.force_epoch, Pf);
        if (rcf) return rcf;
        Pl = &Pf;
    }
    for (int i = 0; i < p.nlaunch; i++) {
        const LinLaunch &l = p.launch[i];
        hipLaunchKernelGGL(lin[l.mode], dim3((unsigned)l.blocks), dim3(l.block), 0, h->stream, *Pl, l.count);
    }
    h->lin_pair_launches += p.pair_launches;
    HIP_TRY(h, hipGetLastError());
    if (p.clear_redo) HIP_TRY(h, hipMemsetAsync(h->d_redo, 0, (size_t)B * redo_words(h->N) * sizeof(int), h->stream));
    HIP_TRY(h, hipEventRecord(ev[1], h->stream));
    h->ptrs.fail_count = h->d_fail_ring + slot;
    HIP_TRY(h, hipMemsetAsync(h->ptrs.fail_count, 0, sizeof(int), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_unconv_ring + slot, 0, sizeof(int), h->stream));
    if (h->d_susp_count) HIP_TRY(h, hipMemsetAsync(h->d_susp_count + slot, 0, sizeof(int), h->stream)); // (hand-over count of this launch)
    if (p.spec_next) {
        // (d_inv: read by the speculative lineariser only, which every later sort of this stream comes behind - ev_spec above)
        if (p.sort_next && sort_into(h, map_buf(p.next_map), h->d_inv)) return USVMPC_E_HIP;
        HIP_TRY(h, hipEventRecord(h->ev_pre, h->stream));
    }
    if (p.copy_iter_prev)
        HIP_TRY(h, hipMemcpyAsync(h->d_iter_prev, h->ptrs.qp_iter, (size_t)h->B * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    if (h->spec.npt != (h->spec.any_bsoft ? k.npt_soft : k.npt_hard)) {
        h->err = "workspace layout mismatch between host and kernels";
        return USVMPC_E_ARG;
    }
    if (!cond && k.qp[SLOT_QP] == nullptr) { h->err = "development build: bench instantiation only"; return USVMPC_E_ARG; }
    const int rcq = cond ? launch_cond(h) : launch_qp(h, k, phase);
    if (rcq) return rcq;
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[2], h->stream));
    if (phase == 0) { // (an RTI solve: one QP per instance)
        hipLaunchKernelGGL(usv_count_unconverged, dim3((B + 255) / 256), dim3(256), 0, h->stream, h->ptrs.qp_status, B,
                           h->d_unconv_ring + slot, h->d_unconv_total);
        HIP_TRY(h, hipGetLastError());
    }
    if (p.spec_next) { // the next tick's lineariser, behind this launch on the second stream, under the map made above
        HIP_TRY(h, hipStreamWaitEvent(h->aux_stream, h->ev_pre, 0));
        DevPtrs Pn = h->ptrs;
        Pn.perm = map_buf(p.next_map);
        Pn.perm_cur = h->ptrs.perm;
        Pn.inv_next = Pn.perm ? h->d_inv : nullptr;
        // (launch_qp has just said whether this launch hands instances over: DevPtrs::susp_count)
        const LinLaunch l = lin_launch(h->sched.launched_ahead(h->ptrs.susp_count != nullptr, p.next_map), pairs, h->N, h->Bp);
        hipLaunchKernelGGL(lin[l.mode], dim3((unsigned)l.blocks), dim3(l.block), 0, h->aux_stream, Pn, l.count);
        if (pairs) h->lin_pair_launches++;
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipEventRecord(h->ev_spec, h->aux_stream));
    }
    h->nsolves++;
    h->world.plan_solved(); // (exchanged plans: the iterate is this solve's)
    h->layout_dirty = false;
    h->last_cond = cond;
    CopyDesc back;
    if (h->hm.read_back(back)) return mirror_copy(h, back, false); // [x | u | status] of this solve, one copy
    return 0;
}

// planes per stage of the packed [B A] for this model (MatPack)
int model_mat_planes(int model)
{
    switch (model) {
#ifndef USV_GEN_ONLY
    case USVMPC_MODEL_USV: return MatPack<ModelM0>::NPK;
    case USVMPC_MODEL_GUIDANCE_CA1: return MatPack<ModelM1>::NPK;
    case USVMPC_MODEL_PF_CA: return MatPack<ModelM2>::NPK;
#endif
#ifdef USV_GEN_MODEL_HEADER
    case USVMPC_MODEL_GENERATED: return MatPack<ModelGen>::NPK;
#endif
    }
    return 0;
}

// planes per stage of the handle's workspace (host_spec.hpp)
int ws_planes(const usvmpc_handle *h)
{
    return usv::ws_planes(h->nx, h->nu, h->kch, h->soft, model_mat_planes(h->desc.model), h->spec.any_bsoft != 0);
}

// whether the model declares the columns the lineariser has to integrate (PairCols: the paired lineariser, option "lin_pairs")
bool model_has_pairs(int model)
{
    switch (model) {
#ifndef USV_GEN_ONLY
    case USVMPC_MODEL_USV: return PairCols<ModelM0>::ENABLED;
    case USVMPC_MODEL_GUIDANCE_CA1: return PairCols<ModelM1>::ENABLED;
    case USVMPC_MODEL_PF_CA: return PairCols<ModelM2>::ENABLED;
#endif
#ifdef USV_GEN_MODEL_HEADER
    case USVMPC_MODEL_GENERATED: return PairCols<ModelGen>::ENABLED;
#endif
    }
    return false;
}

// the kernel table of the handle's model in this library (false: none)
bool model_kernels(const usvmpc_handle *h, Kernels &k)
{
    switch (h->desc.model) {
#ifdef USV_BENCH_ONLY
    case USVMPC_MODEL_PF_CA: if (h->kch <= 1) { k = kernels_for<ModelM2, 1, false>(h); return true; } break;
    case USVMPC_MODEL_GUIDANCE_CA1: if (h->kch <= 1) { k = kernels_for<ModelM1, 1, true>(h); return true; } break;
#elif !defined(USV_GEN_ONLY)
    case USVMPC_MODEL_USV: k = kernels_for<ModelM0, 0, false>(h); return true;
    case USVMPC_MODEL_GUIDANCE_CA1: k = h->kch <= 1 ? kernels_for<ModelM1, 1, true>(h) : kernels_for<ModelM1, 2, true>(h); return true;
    case USVMPC_MODEL_PF_CA: k = h->kch <= 1 ? kernels_for<ModelM2, 1, false>(h) : kernels_for<ModelM2, 2, false>(h); return true;
#endif
#if defined(USV_GEN_MODEL_HEADER) && !defined(USV_BENCH_ONLY)
    case USVMPC_MODEL_GENERATED: k = kernels_for<ModelGen, USV_GEN_KCH, (USV_GEN_SOFT != 0)>(h); return true;
#endif
    }
    return false;
}

int launch(usvmpc_handle *h, int phase = 0)
{
    Kernels k;
    if (!model_kernels(h, k)) { h->err = "unknown model"; return USVMPC_E_ARG; }
    return launch_solve(h, k, phase);
}

// ---- multiplier read-back: buffers on first use, one kernel per solve they are asked for
int ensure_export(usvmpc_handle *h)
{
    if (h->nsolves == 0) { h->err = "no QP has been solved yet: nothing to read back"; return USVMPC_E_ARG; }
    if (h->layout_dirty) { h->err = "the row layout option changed after the last solve: solve again before reading multipliers"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    DevPtrs &P = h->ptrs;
    if (!P.lam_out) {
        P.nlam = lam_len(h->spec, h->soft);
        const size_t cnt = (size_t)h->B * (h->N + 1) * (size_t)(P.nlam > 0 ? P.nlam : 1);
        if (dev_alloc(h, &P.lam_out, cnt, false)) return USVMPC_E_HIP;
        if (dev_alloc(h, &P.t_out, cnt, false)) { P.lam_out = nullptr; return USVMPC_E_HIP; }
        h->export_at = -1;
    }
    if (h->export_at == h->nsolves) return 0;
    if (h->last_cond) {
        // the partially condensed solve keeps its rows in per-workgroup scratch: it writes "lam" / "t" itself, when the buffers exist
        h->err = "\"lam\" / \"t\" of a partially condensed solve (qp_cond_N) are written by the solve itself: the buffers exist from now on "
                 "(option \"keep_multipliers\" = 1 creates them up front) - solve again";
        return USVMPC_E_ARG;
    }
    const size_t nbytes = (size_t)h->B * (h->N + 1) * (size_t)(P.nlam > 0 ? P.nlam : 1) * sizeof(double);
    HIP_TRY(h, hipMemsetAsync(P.lam_out, 0, nbytes, h->stream));
    HIP_TRY(h, hipMemsetAsync(P.t_out, 0, nbytes, h->stream));
    Kernels k;
    if (!model_kernels(h, k)) { h->err = "multiplier read-back: no kernel for this model in this library"; return USVMPC_E_ARG; }
    hipLaunchKernelGGL(k.qp_export, dim3((unsigned)((h->Bp + 3) / 4)), dim3(64), 0, h->stream, h->ptrs, (long)h->Bp);
    HIP_TRY(h, hipGetLastError());
    h->export_at = h->nsolves;
    return 0;
}

} // namespace

// ---------------------------------------------------------------------------------- integrator handle (usvmpc_sim_*)
// B instances of one model's ERK4 over one sampling period (sim.hpp).  Inputs x [B][nx], u [B][nu]; outputs x_next [B][nx] and, with
// sens_forw, S_forw [B][nx][nx + nu].  `owner` tells a plant of THIS library from one made by another build (a generated-model library
// holds other kernels under the same model id).
static const char g_lib_tag = 0;
thread_local std::string g_sim_create_err;

struct usvmpc_sim {
    const void *owner;
    int model, nx, nu, nz, B, device;
    double T;
    int num_steps, sens;
    hipStream_t stream;
    bool own_stream;
    double *x, *u, *xn, *S;   // device
    std::string err;
};

namespace {

#define SIM_TRY(s, call)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (s)->err = std::string(#call) + ": " + hipGetErrorString(e_);                         \
            return USVMPC_E_HIP;                                                                  \
        }                                                                                         \
    } while (0)

int sim_check(const usvmpc_sim_desc &d, int &nx, int &nu, std::string &err)
{
    if (model_dims(d.model, nx, nu)) { err = "unknown model id " + std::to_string(d.model) + " in this library"; return USVMPC_E_ARG; }
#ifdef USV_GEN_ONLY
    if (d.model != USVMPC_MODEL_GENERATED) { err = "this library only holds the generated model"; return USVMPC_E_ARG; }
#endif
    if (d.batch < 1) { err = "batch must be >= 1"; return USVMPC_E_ARG; }
    if (!(d.T > 0.0) || !std::isfinite(d.T)) { err = "T must be positive and finite"; return USVMPC_E_ARG; }
    if (d.num_steps < 1) { err = "num_steps must be >= 1"; return USVMPC_E_ARG; }
    return 0;
}

// the field table of the integrator: device array and its length per instance
double *sim_field(usvmpc_sim *s, const std::string &f, bool set, int &n)
{
    if (f == "x" && set) { n = s->nx; return s->x; }
    if (f == "u" && set) { n = s->nu; return s->u; }
    if (f == "x" && !set) { n = s->nx; return s->xn; }
    if (f == "S_forw" && !set) { n = s->nx * s->nz; return s->S; }
    return nullptr;
}

template <class M>
void sim_launch_model(usvmpc_sim *s)
{
    const long B = s->B;
    if (s->sens) {
        const long threads = B * LANES;
        hipLaunchKernelGGL((usv_sim<M, true>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s->stream, s->x, s->u, s->xn, s->S, B, s->T,
                           s->num_steps);
    } else {
        hipLaunchKernelGGL((usv_sim<M, false>), dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s->stream, s->x, s->u, s->xn, s->S, B, s->T,
                           s->num_steps);
    }
}

} // namespace

// ---------------------------------------------------------------------------------- C ABI
extern "C" {

int usvmpc_model_dims(int model, int *nx, int *nu)
{
    int a, b;
    if (model_dims(model, a, b)) return USVMPC_E_ARG;
    if (nx) *nx = a;
    if (nu) *nu = b;
    return 0;
}

void usvmpc_default_options(usvmpc_desc *d)
{
    if (d) default_options(*d);
}

int usvmpc_hpipm_profile(usvmpc_desc *d, int mode)
{
    return (d && hpipm_profile(*d, mode)) ? 0 : USVMPC_E_ARG;
}

int usvmpc_create(const usvmpc_desc *d, usvmpc_handle **out)
{
    if (!d || !out) return USVMPC_E_ARG;
    *out = nullptr;
    DevSpec S;
    const std::string err = build_spec(*d, S);
    if (!err.empty()) {
        g_create_err = err;
        std::fprintf(stderr, "usvmpc_create: %s\n", err.c_str());
        return USVMPC_E_ARG;
    }
    if (d->model != USVMPC_MODEL_GENERATED && (d->model == USVMPC_MODEL_GUIDANCE_CA1) != (d->soft != 0) && d->K > 0) {
        std::fprintf(stderr, "usvmpc_create: obstacle rows are soft for model 1 and hard for model 2\n");
        return USVMPC_E_ARG;
    }
#ifdef USV_GEN_MODEL_HEADER
    if (d->model == USVMPC_MODEL_GENERATED &&
        ((S.K + LANES - 1) / LANES != USV_GEN_KCH || (S.K > 0 && (d->soft != 0) != (USV_GEN_SOFT != 0)))) {
        std::fprintf(stderr, "usvmpc_create: this library was generated for %d obstacle chunk(s), soft = %d\n", USV_GEN_KCH, USV_GEN_SOFT);
        return USVMPC_E_ARG;
    }
#endif
#ifdef USV_GEN_ONLY
    if (d->model != USVMPC_MODEL_GENERATED) {
        std::fprintf(stderr, "usvmpc_create: this library only holds the generated model\n");
        return USVMPC_E_ARG;
    }
#endif
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || d->device < 0 || d->device >= ndev) {
        std::fprintf(stderr, "usvmpc_create: no usable HIP device (count %d, requested %d); there is no CPU fallback\n",
                     ndev, d->device);
        return USVMPC_E_NODEVICE;
    }
    usvmpc_handle *h = new usvmpc_handle();
    h->desc = *d;
    h->spec = S;
    model_dims(d->model, h->nx, h->nu);
    h->nz = h->nx + h->nu; h->ny = S.ny; h->ny_e = S.ny_e;
    h->N = S.N; h->K = S.K; h->B = S.B; h->Bp = S.Bp;
    h->kch = d->model == USVMPC_MODEL_USV ? 0 : ((S.K + LANES - 1) / LANES > 1 ? 2 : 1);
    h->soft = d->soft != 0 || d->model == USVMPC_MODEL_GUIDANCE_CA1;
#ifdef USV_GEN_MODEL_HEADER
    if (d->model == USVMPC_MODEL_GENERATED) { h->kch = USV_GEN_KCH; h->soft = USV_GEN_SOFT != 0; }
#endif
    // (new usvmpc_handle(): every member zero, nullptr or false unless its declaration says otherwise; the options' defaults: Options)
    h->device = d->device;
    h->opt = Options::defaults(model_has_pairs(h->desc.model));
    h->sched.reset();
    h->caps.reset();
    {
        hipDeviceProp_t prop;
        h->ncu = (hipGetDeviceProperties(&prop, d->device) == hipSuccess) ? prop.multiProcessorCount : 0;
    }
    auto fail = [&](int rc) {
        std::fprintf(stderr, "usvmpc_create: %s\n", h->err.c_str());
        for (void *a : h->allocs) (void)hipFree(a);
        if (h->mirror) (void)hipHostFree(h->mirror);
        delete h;
        return rc;
    };
#define TRY_C(x) do { int rc_ = (x); if (rc_) return fail(rc_); } while (0)
#define HIP_C(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); return fail(USVMPC_E_HIP); } } while (0)
    HIP_C(hipSetDevice(h->device));
    HIP_C(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (int r = 0; r < usvmpc_handle::RING; r++)
        for (int i = 0; i < 4; i++) HIP_C(hipEventCreate(&h->ev[r][i]));
    const size_t B = h->B, N = h->N, K = h->K;
    const size_t stride = (size_t)h->Bp * LANES;
    const size_t kch = h->kch ? h->kch : 1;
    DevPtrs &P = h->ptrs;
    h->spec.npt = ws_planes(h);
    // one stage of the workspace is addressed through ONE 32-bit buffer window (lanes::Planes: group * npt * 128 + ...)
    if ((size_t)h->Bp * (size_t)h->spec.npt * 128u > (size_t)UINT32_MAX - 16384u) { // (16 KB of headroom: a parked row addresses just past the window - qp_ipm.hpp)
        h->err = "batch too large for one handle: batch * " + std::to_string(h->spec.npt * 128) + " bytes per stage exceed the 4 GiB "
                 "buffer window (at most " + std::to_string((size_t)UINT32_MAX / ((size_t)h->spec.npt * 128u) / 4 * 4) + " instances); use several handles";
        return fail(USVMPC_E_ARG);
    }
    TRY_C(dev_alloc(h, &h->d_spec, 1, false));
    HIP_C(hipMemcpy(h->d_spec, &h->spec, sizeof(DevSpec), hipMemcpyHostToDevice));
    P.spec = h->d_spec;
    {   // the caller-visible arrays: one arena [x | u | status | x0 | yref | yref_e | p | lh] (field_plan.hpp)
        const ArenaLayout lay = arena_layout(field_dims(h), B);
        TRY_C(dev_alloc(h, &h->arena, lay.bytes(), true));
        char *a = h->arena;
        P.x = (double *)(a + lay.off[FLD_X]);
        P.u = (double *)(a + lay.off[FLD_U]);
        P.status = (int *)(a + lay.off[FLD_STATUS]);
        P.x0 = (double *)(a + lay.off[FLD_X0]);
        P.yref = (double *)(a + lay.off[FLD_YREF]);
        P.yref_e = (double *)(a + lay.off[FLD_YREF_E]);
        P.p = (double *)(a + lay.off[FLD_P]);
        P.lh = (double *)(a + lay.off[FLD_LH]);
        if (lay.bytes() <= MIRROR_MAX) {
            HIP_C(hipHostMalloc((void **)&h->mirror, lay.bytes(), hipHostMallocDefault));
            std::memset(h->mirror, 0, lay.bytes());
        }
        h->hm.reset(lay, h->mirror != nullptr);
    }
    TRY_C(dev_alloc(h, &P.sl, B * N * K, true));
    TRY_C(dev_alloc(h, &P.su, B * N * K, true));
    TRY_C(dev_alloc(h, &P.pi, B * N * h->nx, true));
    TRY_C(dev_alloc(h, &P.qp_iter, B, true));
    TRY_C(dev_alloc(h, &P.qp_status, B, true));
    TRY_C(dev_alloc(h, &P.res, B * 4, true));
    TRY_C(dev_alloc(h, &P.obs_tmin, B, true));
    TRY_C(dev_alloc(h, &h->d_fail_ring, usvmpc_handle::RING, true));
    TRY_C(dev_alloc(h, &h->d_unconv_ring, usvmpc_handle::RING, true));
    TRY_C(dev_alloc(h, &h->d_unconv_total, 1, true));
    TRY_C(dev_alloc(h, &P.queue, 1, true));
    TRY_C(dev_alloc(h, &P.nlp_res, B * 4, true));
    TRY_C(dev_alloc(h, &P.sqp_iter, B, true));
    TRY_C(dev_alloc(h, &P.sqp_state, B, true));
    TRY_C(dev_alloc(h, &P.sqp_running, 1, true));
    TRY_C(dev_alloc(h, &h->d_perm, B, true));
    TRY_C(dev_alloc(h, &h->d_iter_prev, B, true));
    TRY_C(dev_alloc(h, &h->d_hist, SORT_BINS, true));
    TRY_C(dev_alloc(h, &h->d_cursor, SORT_BINS, true));
    TRY_C(dev_alloc(h, &P.ws, (N + 1) * (size_t)ws_planes(h) * stride, true));
    HIP_C(hipDeviceSynchronize());
#undef TRY_C
#undef HIP_C
    *out = h;
    return 0;
}

int usvmpc_destroy(usvmpc_handle *h)
{
    if (!h) return USVMPC_E_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->aux_stream) {
        (void)hipStreamSynchronize(h->aux_stream);
        (void)hipStreamDestroy(h->aux_stream);
    }
    if (h->ev_pre) (void)hipEventDestroy(h->ev_pre);
    if (h->ev_spec) (void)hipEventDestroy(h->ev_spec);
    co_release(h);
    for (void *a : h->allocs) (void)hipFree(a);
    if (h->mirror) (void)hipHostFree(h->mirror);
    for (int r = 0; r < usvmpc_handle::RING; r++)
        for (int i = 0; i < 4; i++)
            if (h->ev[r][i]) (void)hipEventDestroy(h->ev[r][i]);
    if (h->own_stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

int usvmpc_set(usvmpc_handle *h, const char *field, int stage, const double *v, size_t n)
{
    return copy_field(h, field, stage, const_cast<double *>(v), n, true);
}

int usvmpc_get(usvmpc_handle *h, const char *field, int stage, double *out, size_t n)
{
    return copy_field(h, field, stage, out, n, false);
}

int usvmpc_get_int(usvmpc_handle *h, const char *field, int *out)
{
    if (!h || !out) return USVMPC_E_ARG;
    const FieldRow *row = find_field(field);
    if (!row || !(row->rights & R_GET_INT)) { h->err = std::string("unknown integer field '") + (field ? field : "") + "'"; return USVMPC_E_FIELD; }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(out, field_ptr(h, row->id), (size_t)h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int usvmpc_solve_async(usvmpc_handle *h)
{
    if (!h) return USVMPC_E_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch(h);
}

int usvmpc_sync(usvmpc_handle *h)
{
    if (!h) return USVMPC_E_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->sched.outstanding) { // (the lineariser that runs a tick ahead is part of the work enqueued so far)
        HIP_TRY(h, hipStreamSynchronize(h->aux_stream));
        h->sched.synced();
    }
    h->hm.synced();
    return 0;
}

int usvmpc_solve(usvmpc_handle *h, int *status)
{
    int rc = usvmpc_solve_async(h);
    if (rc) return rc;
    rc = usvmpc_sync(h);
    if (rc) return rc;
    int worst = 0;
    if (status) {
        if (h->hm.get_served(FLD_STATUS)) std::memcpy(status, h->mirror + h->hm.lay.off[FLD_STATUS], (size_t)h->B * sizeof(int)); // (came back with x | u)
        else {
            rc = usvmpc_get_int(h, "status", status);
            if (rc) return rc;
        }
        for (int b = 0; b < h->B; b++) worst = status[b] > worst ? status[b] : worst;
    }
    return worst;
}

int usvmpc_solve_sqp(usvmpc_handle *h, int *status)
{
    if (!h) return USVMPC_E_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    const int B = h->B;
    const int max_iter = h->desc.nlp_max_iter > 0 ? h->desc.nlp_max_iter : 100;
    {
        const int rcs = spec_cancel(h);
        if (rcs) return rcs;
    }
    hipLaunchKernelGGL(usv_sqp_begin, dim3((B + 255) / 256), dim3(256), 0, h->stream, h->ptrs, B);
    HIP_TRY(h, hipGetLastError());
    for (int it = 0; it < max_iter; it++) {
        HIP_TRY(h, hipMemsetAsync(h->ptrs.sqp_running, 0, sizeof(int), h->stream));
        // the very first launch of a handle has no multipliers yet; afterwards the workspace holds those of the
        // last QP of every instance (acados likewise keeps nlp_out between calls)
        // ... unless the group -> instance map has changed since (difficulty binning re-sorted or switched off): the
        // workspace is group-indexed, so the multipliers there belong to other instances and the call starts from
        // zero multipliers like a first one
        const bool fresh = it == 0 && (h->nsolves == 0 || h->map_changed);
        if (it == 0) h->map_changed = false;
        const int rc = launch(h, fresh ? 1 : 2);
        if (rc) return rc;
        int running = 0;
        HIP_TRY(h, hipMemcpyAsync(&running, h->ptrs.sqp_running, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (running == 0) break; // every instance has converged or failed
    }
    hipLaunchKernelGGL(usv_sqp_end, dim3((B + 255) / 256), dim3(256), 0, h->stream, h->ptrs, B);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int worst = 0;
    if (status) {
        const int rc = usvmpc_get_int(h, "status", status);
        if (rc) return rc;
        for (int b = 0; b < B; b++) worst = status[b] > worst ? status[b] : worst;
    }
    return worst;
}

int usvmpc_get_device_ptr(usvmpc_handle *h, const char *field, void **dptr)
{
    if (!h || !dptr) return USVMPC_E_ARG;
    if (field && std::strcmp(field, "cost_tracked") == 0) { // (no field of the table: it exists only while tracking runs)
        if (!h->d_cost_sum) { h->err = "cost_tracked: no tracking is running (usvmpc_cost_track)"; return USVMPC_E_ARG; }
        *dptr = h->d_cost_sum;
        return 0;
    }
    const FieldRow *row = find_field(field);
    if (!row || !(row->rights & R_DEV)) { h->err = std::string("unknown field '") + (field ? field : "") + "'"; return USVMPC_E_FIELD; }
    if (row->flags & FF_COST) {
        // cost memory only: nothing a lineariser reads and nothing the host mirror holds is exposed - the pipeline keeps running
        int rcc = cost_check(h);
        if (rcc) return rcc;
        rcc = cost_alloc(h);
        if (rcc) return rcc;
        *dptr = field_ptr(h, row->id);
        return 0;
    }
    if (row->flags & FF_TRACK) {
        // a track field: the caller's own kernels may move the obstacles behind the handle's back, so the prediction runs before every solve
        // from now on.  Nothing a lineariser reads is exposed: the pipeline keeps running.
        const int rca = tracks_alloc(h);
        if (rca) return rca;
        h->tracks_extern = true;
        if (row->id == FLD_OBS_POS) h->tracks_pos_set = true;
        *dptr = field_ptr(h, row->id);
        return 0;
    }
    if (row->flags & FF_PF) h->pf_stale = true; // (the caller may write the rows behind the path-following front end's back)
    {   // the caller is about to read (or write) device memory directly: pending host writes go up, and the host mirror no longer
        // vouches for the device's x / u
        HIP_TRY(h, hipSetDevice(h->device));
        const int rcf = mirror_flush(h);
        if (rcf) return rcf;
        h->hm.handed_out();
        if (row->id == FLD_X) h->world.plan_lost(); // (exchanged plans: the caller may write the iterate behind the library's back)
        const int rcs = spec_cancel(h); // (and no lineariser runs ahead on arrays the caller may write behind the library's back)
        if (rcs) return rcs;
    }
    *dptr = field_ptr(h, row->id);
    return 0;
}

int usvmpc_kernel_ms(usvmpc_handle *h, int n, float *linearize_ms, float *qp_ms)
{
    if (!h || n < 1) return USVMPC_E_ARG;
    if (h->nsolves < n || n > usvmpc_handle::RING) { h->err = "fewer solves recorded than requested"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    for (int i = 0; i < n; i++) { // oldest of the last n first
        hipEvent_t *ev = h->ev[(h->nsolves - n + i) % usvmpc_handle::RING];
        HIP_TRY(h, hipEventSynchronize(ev[2]));
        float a = 0, b = 0;
        HIP_TRY(h, hipEventElapsedTime(&a, ev[0], ev[1]));
        HIP_TRY(h, hipEventElapsedTime(&b, ev[1], ev[2]));
        if (linearize_ms) linearize_ms[i] = a;
        if (qp_ms) qp_ms[i] = b;
    }
    return 0;
}

int usvmpc_followup_ms(usvmpc_handle *h, int n, float *ms)
{
    if (!h || n < 1 || !ms) return USVMPC_E_ARG;
    if (h->nsolves < n || n > usvmpc_handle::RING) { h->err = "fewer solves recorded than requested"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    for (int i = 0; i < n; i++) { // oldest of the last n first
        const int r = (h->nsolves - n + i) % usvmpc_handle::RING;
        ms[i] = 0.0f;
        if (!h->ev3_set[r]) continue;
        HIP_TRY(h, hipEventSynchronize(h->ev[r][2]));
        HIP_TRY(h, hipEventElapsedTime(&ms[i], h->ev[r][3], h->ev[r][2]));
    }
    return 0;
}

int usvmpc_tick_ms(usvmpc_handle *h, int n, float *ms)
{
    if (!h || n < 2 || !ms) return USVMPC_E_ARG;
    if (h->nsolves < n || n > usvmpc_handle::RING) { h->err = "fewer solves recorded than requested"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    for (int i = 0; i + 1 < n; i++) { // oldest of the last n first
        hipEvent_t *ev = h->ev[(h->nsolves - n + i) % usvmpc_handle::RING], *evn = h->ev[(h->nsolves - n + i + 1) % usvmpc_handle::RING];
        HIP_TRY(h, hipEventSynchronize(evn[0]));
        HIP_TRY(h, hipEventElapsedTime(&ms[i], ev[0], evn[0]));
    }
    return 0;
}

// x_start == nullptr: M::fjvp at x (usv_debug_model); otherwise ModelCall<M>::prepare(x_start), then ModelCall<M>::fjvp at x (usv_debug_model_from)
static int debug_model_eval(int model, int device, int n, const double *x_start, const double *x, const double *u, double *f, double *J)
{
    int nx, nu;
    if (model_dims(model, nx, nu) || n < 1 || !x || !f || !J || (nu > 0 && !u)) return USVMPC_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return USVMPC_E_NODEVICE;
    const int nz = nx + nu;
    double *dx0 = nullptr, *dx = nullptr, *du = nullptr, *df = nullptr, *dJ = nullptr;
    int rc = 0;
    if (hipMalloc((void **)&dx, sizeof(double) * n * nx) != hipSuccess || hipMalloc((void **)&du, sizeof(double) * n * (nu ? nu : 1)) != hipSuccess ||
        hipMalloc((void **)&df, sizeof(double) * n * nx) != hipSuccess || hipMalloc((void **)&dJ, sizeof(double) * n * nx * nz) != hipSuccess ||
        (x_start && hipMalloc((void **)&dx0, sizeof(double) * n * nx) != hipSuccess))
        rc = USVMPC_E_HIP;
    if (!rc) {
        (void)hipMemcpy(dx, x, sizeof(double) * n * nx, hipMemcpyHostToDevice);
        if (x_start) (void)hipMemcpy(dx0, x_start, sizeof(double) * n * nx, hipMemcpyHostToDevice);
        if (nu) (void)hipMemcpy(du, u, sizeof(double) * n * nu, hipMemcpyHostToDevice);
        const dim3 grid((unsigned)((n * nz + 63) / 64)), block(64);
#define USV_DEBUG_LAUNCH(M) \
    if (x_start) hipLaunchKernelGGL(usv_debug_model_from<M>, grid, block, 0, 0, n, dx0, dx, du, df, dJ); \
    else hipLaunchKernelGGL(usv_debug_model<M>, grid, block, 0, 0, n, dx, du, df, dJ)
        switch (model) {
#ifndef USV_GEN_ONLY
        case USVMPC_MODEL_USV: USV_DEBUG_LAUNCH(ModelM0); break;
        case USVMPC_MODEL_GUIDANCE_CA1: USV_DEBUG_LAUNCH(ModelM1); break;
        case USVMPC_MODEL_PF_CA: USV_DEBUG_LAUNCH(ModelM2); break;
#endif
#ifdef USV_GEN_MODEL_HEADER
        case USVMPC_MODEL_GENERATED: USV_DEBUG_LAUNCH(ModelGen); break;
#endif
        default: rc = USVMPC_E_ARG;
        }
#undef USV_DEBUG_LAUNCH
        if (!rc && (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)) rc = USVMPC_E_HIP;
        if (!rc) {
            (void)hipMemcpy(f, df, sizeof(double) * n * nx, hipMemcpyDeviceToHost);
            (void)hipMemcpy(J, dJ, sizeof(double) * n * nx * nz, hipMemcpyDeviceToHost);
        }
    }
    (void)hipFree(dx0); (void)hipFree(dx); (void)hipFree(du); (void)hipFree(df); (void)hipFree(dJ);
    return rc;
}

int usvmpc_debug_model_eval(int model, int device, int n, const double *x, const double *u, double *f, double *J)
{
    return debug_model_eval(model, device, n, nullptr, x, u, f, J);
}

int usvmpc_debug_model_eval_from(int model, int device, int n, const double *x_start, const double *x, const double *u, double *f, double *J)
{
    if (!x_start) return USVMPC_E_ARG;
    return debug_model_eval(model, device, n, x_start, x, u, f, J);
}

int usvmpc_debug_fast_math(int device, int n, const double *x, double *rcp, double *rsq)
{
    if (n < 1 || !x || !rcp || !rsq) return USVMPC_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return USVMPC_E_NODEVICE;
    double *dx = nullptr, *drcp = nullptr, *drsq = nullptr;
    int rc = 0;
    if (hipMalloc((void **)&dx, sizeof(double) * n) != hipSuccess || hipMalloc((void **)&drcp, sizeof(double) * n) != hipSuccess ||
        hipMalloc((void **)&drsq, sizeof(double) * n) != hipSuccess)
        rc = USVMPC_E_HIP;
    if (!rc) {
        (void)hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(usv_debug_fast_math, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, n, dx, drcp, drsq);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = USVMPC_E_HIP;
        if (!rc) {
            (void)hipMemcpy(rcp, drcp, sizeof(double) * n, hipMemcpyDeviceToHost);
            (void)hipMemcpy(rsq, drsq, sizeof(double) * n, hipMemcpyDeviceToHost);
        }
    }
    (void)hipFree(dx); (void)hipFree(drcp); (void)hipFree(drsq);
    return rc;
}

int usvmpc_debug_lanes(int device, int ngroups, int block_threads, const double *in, const int *iin, double *out, int *iout, double *planes, long planes_doubles)
{
    namespace lp = lanes_probe;
    if (ngroups < 1 || ngroups > (1 << 20) || (block_threads != 64 && block_threads != 256) || !in || !iin || !out || !iout || !planes ||
        planes_doubles < 2L * lp::PL_PAD + (long)ngroups * lp::NPL * 16)
        return USVMPC_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return USVMPC_E_NODEVICE;
    const size_t n_in = sizeof(double) * ngroups * lp::NIN * 16, n_iin = sizeof(int) * ngroups * lp::NIIN * 16, n_out = sizeof(double) * ngroups * lp::NOUT * 16,
                 n_iout = sizeof(int) * ngroups * lp::NIOUT * 16, n_pl = sizeof(double) * (size_t)planes_doubles;
    double *din = nullptr, *dout = nullptr, *dpl = nullptr;
    int *diin = nullptr, *diout = nullptr;
    int rc = 0;
    if (hipMalloc((void **)&din, n_in) != hipSuccess || hipMalloc((void **)&diin, n_iin) != hipSuccess || hipMalloc((void **)&dout, n_out) != hipSuccess ||
        hipMalloc((void **)&diout, n_iout) != hipSuccess || hipMalloc((void **)&dpl, n_pl) != hipSuccess)
        rc = USVMPC_E_HIP;
    if (!rc) {
        (void)hipMemcpy(din, in, n_in, hipMemcpyHostToDevice);
        (void)hipMemcpy(diin, iin, n_iin, hipMemcpyHostToDevice);
        (void)hipMemcpy(dout, out, n_out, hipMemcpyHostToDevice);
        (void)hipMemcpy(diout, iout, n_iout, hipMemcpyHostToDevice);
        (void)hipMemcpy(dpl, planes, n_pl, hipMemcpyHostToDevice);
        const lp::Args a{din, diin, dout, diout, dpl, ngroups};
        const int rows = block_threads / 16;
        const dim3 grid((unsigned)((ngroups + rows - 1) / rows)), block((unsigned)block_threads);
        const size_t lds = sizeof(double) * rows * lp::NPL_LDS * 16;
        if (block_threads == 64) hipLaunchKernelGGL(usv_debug_lanes<1>, grid, block, lds, 0, a);
        else hipLaunchKernelGGL(usv_debug_lanes<4>, grid, block, lds, 0, a);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = USVMPC_E_HIP;
        if (!rc) {
            (void)hipMemcpy(out, dout, n_out, hipMemcpyDeviceToHost);
            (void)hipMemcpy(iout, diout, n_iout, hipMemcpyDeviceToHost);
            (void)hipMemcpy(planes, dpl, n_pl, hipMemcpyDeviceToHost);
        }
    }
    (void)hipFree(din); (void)hipFree(diin); (void)hipFree(dout); (void)hipFree(diout); (void)hipFree(dpl);
    return rc;
}

int usvmpc_debug_obstacle_eval(int device, int n, int K, const double *pos, const double *p, double *h, double *grad)
{
    if (n < 1 || K < 1 || !pos || !p || !h || !grad) return USVMPC_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return USVMPC_E_NODEVICE;
    double *dpos = nullptr, *dp = nullptr, *dh = nullptr, *dg = nullptr;
    int rc = 0;
    if (hipMalloc((void **)&dpos, sizeof(double) * n * 2) != hipSuccess || hipMalloc((void **)&dp, sizeof(double) * n * 2 * K) != hipSuccess ||
        hipMalloc((void **)&dh, sizeof(double) * n * K) != hipSuccess || hipMalloc((void **)&dg, sizeof(double) * n * K * 2) != hipSuccess)
        rc = USVMPC_E_HIP;
    if (!rc) {
        (void)hipMemcpy(dpos, pos, sizeof(double) * n * 2, hipMemcpyHostToDevice);
        (void)hipMemcpy(dp, p, sizeof(double) * n * 2 * K, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(usv_debug_obstacle, dim3((unsigned)((n * K + 63) / 64)), dim3(64), 0, 0, n, K, dpos, dp, dh, dg);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = USVMPC_E_HIP;
        if (!rc) {
            (void)hipMemcpy(h, dh, sizeof(double) * n * K, hipMemcpyDeviceToHost);
            (void)hipMemcpy(grad, dg, sizeof(double) * n * K * 2, hipMemcpyDeviceToHost);
        }
    }
    (void)hipFree(dpos); (void)hipFree(dp); (void)hipFree(dh); (void)hipFree(dg);
    return rc;
}

int usvmpc_fail_counts(usvmpc_handle *h, int n, int *counts)
{
    if (!h || n < 1 || !counts) return USVMPC_E_ARG;
    if (h->nsolves < n || n > usvmpc_handle::RING) { h->err = "fewer solves recorded than requested"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    int ring[usvmpc_handle::RING];
    HIP_TRY(h, hipMemcpyAsync(ring, h->d_fail_ring, sizeof(ring), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; i++) counts[i] = ring[(h->nsolves - n + i) % usvmpc_handle::RING];
    return 0;
}

int usvmpc_unconverged_counts(usvmpc_handle *h, int n, int *counts)
{
    if (!h || n < 1 || !counts) return USVMPC_E_ARG;
    if (h->nsolves < n || n > usvmpc_handle::RING) { h->err = "fewer solves recorded than requested"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    int ring[usvmpc_handle::RING];
    HIP_TRY(h, hipMemcpyAsync(ring, h->d_unconv_ring, sizeof(ring), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; i++) counts[i] = ring[(h->nsolves - n + i) % usvmpc_handle::RING];
    return 0;
}

int usvmpc_unconverged_total(usvmpc_handle *h, long long *total)
{
    if (!h || !total) return USVMPC_E_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    unsigned long long v = 0;
    HIP_TRY(h, hipMemcpyAsync(&v, h->d_unconv_total, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *total = (long long)v;
    return 0;
}

int usvmpc_handover_counts(usvmpc_handle *h, int n, int *counts)
{
    if (!h || n < 1 || !counts) return USVMPC_E_ARG;
    if (h->nsolves < n || n > usvmpc_handle::RING) { h->err = "fewer solves recorded than requested"; return USVMPC_E_ARG; }
    if (!h->d_susp_count) { for (int i = 0; i < n; i++) counts[i] = 0; return 0; } // (no launch of this handle has handed anything over)
    HIP_TRY(h, hipSetDevice(h->device));
    int ring[usvmpc_handle::RING];
    HIP_TRY(h, hipMemcpyAsync(ring, h->d_susp_count, sizeof(ring), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; i++) counts[i] = ring[(h->nsolves - n + i) % usvmpc_handle::RING];
    return 0;
}

int usvmpc_handover_co_counts(usvmpc_handle *h, int n, int *finished, int *timeouts)
{
    if (!h || n < 1 || !finished) return USVMPC_E_ARG;
    if (h->nsolves < n || n > usvmpc_handle::RING) { h->err = "fewer solves recorded than requested"; return USVMPC_E_ARG; }
    for (int i = 0; i < n; i++) { finished[i] = 0; if (timeouts) timeouts[i] = 0; }
    if (!h->d_co_ctl) return 0; // (no launch of this handle had a co-resident follow-up kernel)
    HIP_TRY(h, hipSetDevice(h->device));
    int ring[usvmpc_handle::RING * 8];
    HIP_TRY(h, hipMemcpyAsync(ring, h->d_co_ctl, sizeof(ring), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; i++) {
        const int r = (h->nsolves - n + i) % usvmpc_handle::RING;
        finished[i] = ring[8 * r + 3];
        if (timeouts) timeouts[i] = ring[8 * r + 4];
    }
    return 0;
}

int usvmpc_pipeline_stats(usvmpc_handle *h, long *used, long *discarded)
{
    if (!h) return USVMPC_E_ARG;
    if (used) *used = h->sched.hits;
    if (discarded) *discarded = h->sched.misses;
    return 0;
}

int usvmpc_lin_pair_launches(usvmpc_handle *h, long *launches)
{
    if (!h || !launches) return USVMPC_E_ARG;
    *launches = h->lin_pair_launches;
    return 0;
}

int usvmpc_last_mapping(usvmpc_handle *h, int *mapping)
{
    if (!h || !mapping) return USVMPC_E_ARG;
    *mapping = h->last_wide;
    return 0;
}

int usvmpc_last_kernel_ms(usvmpc_handle *h, float *linearize_ms, float *qp_ms)
{
    return usvmpc_kernel_ms(h, 1, linearize_ms, qp_ms);
}

static int apply_static(usvmpc_handle *h);
static int world_step(usvmpc_handle *h, double T);

// ---- the closed-loop log: log_plan.hpp says what a hand-over does and what a read copies; here: the buffers, the launch, the copies
static void log_release(usvmpc_handle *h)
{
    const LogLayout &l = h->log.lay;
    dev_free(h, h->log_x, (size_t)l.x_bytes);
    dev_free(h, h->log_u, (size_t)l.u_bytes);
    dev_free(h, h->log_status, (size_t)l.status_bytes);
    dev_free(h, h->log_sums, (size_t)l.sums_bytes);
    h->log_x = h->log_u = h->log_sums = nullptr;
    h->log_status = nullptr;
}

// a hand-over of a handle whose log runs (usvmpc_advance / usvmpc_advance_sim, behind the mirror's upload and ahead of their own kernel)
static int log_handover(usvmpc_handle *h)
{
    const LogTick t = h->log.on_handover();
    if (t.slot < 0 && !t.errors) return 0;
    const LogLayout &l = h->log.lay;
    LogRec r = h->log_rec;
    r.x0 = h->ptrs.x0; r.u = h->ptrs.u; r.status = h->ptrs.status; r.qp_iter = h->ptrs.qp_iter;
    long n = 0;
    if (t.slot >= 0) {
        const long at = (long)t.slot * l.B;
        if (h->log_x) { r.rx = h->log_x + at * l.nsel; n = std::max(n, (long)l.B * l.nsel); }
        if (h->log_u) { r.ru = h->log_u + at * l.nu; n = std::max(n, (long)l.B * l.nu); }
        if (h->log_status) { r.rs = h->log_status + at; n = std::max(n, (long)l.B); }
    }
    if (t.errors) {
        r.sum_abs = h->log_sums;
        r.sum_sq = h->log_sums + (long)l.B * l.n_err;
        n = std::max(n, (long)l.B * l.n_err);
    }
    hipLaunchKernelGGL(usv_log_record, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, r);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

int usvmpc_log_start(usvmpc_handle *h, const usvmpc_log_desc *d)
{
    if (!h) return USVMPC_E_ARG;
    if (!d) { h->err = "log_start: null descriptor"; return USVMPC_E_ARG; }
    if (h->log.on) { h->err = "log_start: a log is running (usvmpc_log_stop first)"; return USVMPC_E_ARG; }
    LogDesc ld = {};
    ld.capacity = d->capacity; ld.every = d->every; ld.first = d->first; ld.state_mask = d->state_mask;
    ld.record_u = d->record_u; ld.record_status = d->record_status; ld.n_err = d->n_err; ld.err_first = d->err_first;
    for (int c = 0; c < LOG_ERR_MAX; c++) { ld.err_a[c] = d->err_a[c]; ld.err_b[c] = d->err_b[c]; ld.err_c[c] = d->err_c[c]; }
    LogLayout lay;
    if (const char *why = check_log_desc(ld, h->nx, h->nu, h->B, &lay)) { h->err = why; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    // all four buffers or none: a failed allocation leaves the handle as it was
    void *buf[4] = {nullptr, nullptr, nullptr, nullptr};
    const long long want[4] = {lay.x_bytes, lay.u_bytes, lay.status_bytes, lay.sums_bytes};
    for (int i = 0; i < 4; i++) {
        if (want[i] == 0) continue;
        const hipError_t e = hipMalloc(&buf[i], (size_t)want[i]);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            for (int j = 0; j < i; j++)
                if (buf[j]) (void)hipFree(buf[j]);
            h->err = std::string("log_start: hipMalloc of ") + std::to_string(want[i]) + " bytes: " + hipGetErrorString(e);
            return USVMPC_E_HIP;
        }
    }
    for (int i = 0; i < 4; i++)
        if (buf[i]) { h->allocs.push_back(buf[i]); h->bytes += (size_t)want[i]; }
    h->log_x = (double *)buf[0]; h->log_u = (double *)buf[1]; h->log_status = (int *)buf[2]; h->log_sums = (double *)buf[3];
    h->log.start(ld, lay);
    if (h->log_sums) HIP_TRY(h, hipMemsetAsync(h->log_sums, 0, (size_t)lay.sums_bytes, h->stream));
    LogRec r = {};
    r.B = h->B; r.nx = h->nx; r.nu = lay.nu; r.ustride = h->N * h->nu; r.n_err = lay.n_err;
    r.sel = log_pack_mask(ld.state_mask, &r.nsel);
    int eb[LOG_ERR_MAX];
    for (int c = 0; c < LOG_ERR_MAX; c++) {
        eb[c] = ld.err_b[c] < 0 ? 0 : ld.err_b[c];
        if (c < ld.n_err && ld.err_b[c] < 0) r.err_const |= 1u << c;
    }
    r.err_a = log_pack_list(ld.err_a, ld.n_err);
    r.err_b = log_pack_list(eb, ld.n_err);
    r.c0 = ld.err_c[0]; r.c1 = ld.err_c[1]; r.c2 = ld.err_c[2]; r.c3 = ld.err_c[3];
    h->log_rec = r;
    return 0;
}

int usvmpc_log_stop(usvmpc_handle *h)
{
    if (!h) return USVMPC_E_ARG;
    if (!h->log.on) { h->err = "log_stop: no log is running"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    log_release(h);
    h->log.stop();
    return 0;
}

int usvmpc_log_info(usvmpc_handle *h, int *records, long long *handovers, long long *missed, int *nsel)
{
    if (!h) return USVMPC_E_ARG;
    if (!h->log.on) { h->err = "log_info: no log is running (usvmpc_log_start)"; return USVMPC_E_ARG; }
    if (records) *records = h->log.records;
    if (handovers) *handovers = h->log.handovers;
    if (missed) *missed = h->log.missed;
    if (nsel) *nsel = h->log.lay.nsel;
    return 0;
}

int usvmpc_log_read(usvmpc_handle *h, const char *channel, int rec0, int nrec, int b0, int nb, void *out, size_t bytes)
{
    if (!h) return USVMPC_E_ARG;
    LogCopy c;
    if (const char *why = h->log.read_desc(channel, rec0, nrec, b0, nb, &c)) { h->err = why; return USVMPC_E_ARG; }
    if (!out || (long long)bytes != c.bytes()) {
        h->err = "log_read: out must hold exactly " + std::to_string(c.bytes()) + " bytes ([nrec][nb][" + std::to_string(c.n) + "])";
        return USVMPC_E_ARG;
    }
    const char *src = c.channel == LOG_X ? (const char *)h->log_x : c.channel == LOG_U ? (const char *)h->log_u : (const char *)h->log_status;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpy2DAsync(out, (size_t)c.width, src + c.offset, (size_t)c.pitch, (size_t)c.width, (size_t)c.rows, hipMemcpyDeviceToHost,
                                h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int usvmpc_log_errors(usvmpc_handle *h, double *sum_abs, double *sum_sq, long long *count)
{
    if (!h) return USVMPC_E_ARG;
    if (!h->log.on || h->log.lay.n_err == 0) { h->err = "log_errors: no log with error channels is running"; return USVMPC_E_ARG; }
    const size_t half = (size_t)h->log.lay.sums_bytes / 2;
    HIP_TRY(h, hipSetDevice(h->device));
    if (sum_abs) HIP_TRY(h, hipMemcpyAsync(sum_abs, h->log_sums, half, hipMemcpyDeviceToHost, h->stream));
    if (sum_sq) HIP_TRY(h, hipMemcpyAsync(sum_sq, (const char *)h->log_sums + half, half, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (count) *count = h->log.err_count;
    return 0;
}

int usvmpc_log_device_ptr(usvmpc_handle *h, const char *channel, void **dptr)
{
    if (!h || !dptr) return USVMPC_E_ARG;
    if (!h->log.on) { h->err = "log_device_ptr: no log is running (usvmpc_log_start)"; return USVMPC_E_ARG; }
    const std::string s = channel ? channel : "";
    void *p = s == "x" ? (void *)h->log_x : s == "u" ? (void *)h->log_u : s == "status" ? (void *)h->log_status
            : s == "sum_abs" ? (void *)h->log_sums
            : s == "sum_sq" ? (void *)(h->log_sums ? h->log_sums + (long)h->log.lay.B * h->log.lay.n_err : nullptr) : nullptr;
    if (!p) { h->err = "log_device_ptr: '" + s + "' is no channel of the running log"; return USVMPC_E_ARG; }
    *dptr = p;
    return 0;
}

// ---- the objective value: usv_cost_eval on demand, the realised closed-loop cost hand-over by hand-over
int usvmpc_eval_cost(usvmpc_handle *h)
{
    if (!h) return USVMPC_E_ARG;
    return cost_enqueue(h);
}

int usvmpc_cost_track(usvmpc_handle *h, int on)
{
    if (!h) return USVMPC_E_ARG;
    const int rcc = cost_check(h);
    if (rcc) return rcc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (!on) {
        if (h->d_cost_sum) dev_free(h, h->d_cost_sum, (size_t)h->B * sizeof(double));
        h->d_cost_sum = nullptr;
        return 0;
    }
    const int rct = cost_tab_ensure(h);
    if (rct) return rct;
    if (!h->d_cost_sum) {
        double *s = nullptr;
        if (dev_alloc(h, &s, (size_t)h->B, false)) return USVMPC_E_HIP;
        h->d_cost_sum = s;
    }
    HIP_TRY(h, hipMemsetAsync(h->d_cost_sum, 0, (size_t)h->B * sizeof(double), h->stream)); // (behind the hand-overs already enqueued)
    h->cost_count = 0;
    return 0;
}

int usvmpc_cost_tracked(usvmpc_handle *h, double *sum, long long *count)
{
    if (!h) return USVMPC_E_ARG;
    if (!h->d_cost_sum) { h->err = "cost_tracked: no tracking is running (usvmpc_cost_track)"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    if (sum) HIP_TRY(h, hipMemcpyAsync(sum, h->d_cost_sum, (size_t)h->B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (count) *count = h->cost_count;
    return 0;
}

// one step of the tracked sum outside a hand-over: for loops that never call usvmpc_advance (a cascade's two solvers)
int usvmpc_cost_track_now(usvmpc_handle *h)
{
    if (!h) return USVMPC_E_ARG;
    if (!h->d_cost_sum) { h->err = "cost_track_now: no tracking is running (usvmpc_cost_track)"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    {
        const int rcf = mirror_flush(h);
        if (rcf) return rcf;
    }
    return cost_handover(h);
}

int usvmpc_advance(usvmpc_handle *h, double sigma, unsigned long long seed)
{
    if (!h) return USVMPC_E_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    {
        const int rcf = mirror_flush(h);
        if (rcf) return rcf;
    }
    if (h->log.on) { // (ahead of the kernel that overwrites x0)
        const int rcl = log_handover(h);
        if (rcl) return rcl;
    }
    if (h->d_cost_sum) { // (likewise: c_0 of the state the solve saw)
        const int rcc = cost_handover(h);
        if (rcc) return rcc;
    }
    const long n = (long)h->B * h->nx;
    hipLaunchKernelGGL(usv_advance, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->ptrs, h->nx, sigma, seed, h->opt.noise_mask,
                       h->opt.instance_offset);
    HIP_TRY(h, hipGetLastError());
    h->world.plan_handed_over();
    if (h->opt.tracks_on && h->opt.step_on_advance) return tracks_step(h, h->spec.dt); // (the world moves with the vehicle: one shooting interval)
    if (h->world.steps_on_advance(h->opt.step_on_advance != 0)) return world_step(h, h->spec.dt); // (the front end's world likewise)
    return 0;
}

int usvmpc_obstacles_step(usvmpc_handle *h, double T)
{
    if (!h) return USVMPC_E_ARG;
    if (h->K == 0) { h->err = "obstacles_step: this model has no obstacle rows (K = 0)"; return USVMPC_E_FIELD; }
    return tracks_step(h, T);
}

int usvmpc_advance_sim(usvmpc_handle *h, const usvmpc_sim *plant, double sigma, unsigned long long seed)
{
    if (!h) return USVMPC_E_ARG;
    if (!plant) { h->err = "advance_sim: null plant"; return USVMPC_E_ARG; }
    if (plant->owner != &g_lib_tag) {
        h->err = "advance_sim: the plant was created by another solver library (its model's kernels are not in this one)";
        return USVMPC_E_ARG;
    }
    if (plant->model != h->desc.model || plant->nx != h->nx || plant->nu != h->nu) {
        h->err = "advance_sim: the plant's model (" + std::to_string(plant->model) + ", nx " + std::to_string(plant->nx) +
                 ") differs from the solver's (" + std::to_string(h->desc.model) + ", nx " + std::to_string(h->nx) + ")";
        return USVMPC_E_ARG;
    }
    if (plant->device != h->device) {
        h->err = "advance_sim: the plant is on device " + std::to_string(plant->device) + ", the solver on device " + std::to_string(h->device);
        return USVMPC_E_ARG;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    {
        const int rcf = mirror_flush(h);
        if (rcf) return rcf;
    }
    if (h->log.on) { // (ahead of the kernel that overwrites x0)
        const int rcl = log_handover(h);
        if (rcl) return rcl;
    }
    if (h->d_cost_sum) {
        const int rcc = cost_handover(h);
        if (rcc) return rcc;
    }
    const dim3 grid((unsigned)((h->B + 255) / 256)), block(256);
    switch (h->desc.model) {
#ifndef USV_GEN_ONLY
    case USVMPC_MODEL_USV:
        hipLaunchKernelGGL(usv_advance_sim<ModelM0>, grid, block, 0, h->stream, h->ptrs, plant->T, plant->num_steps, sigma, seed, h->opt.noise_mask, h->opt.instance_offset);
        break;
    case USVMPC_MODEL_GUIDANCE_CA1:
        hipLaunchKernelGGL(usv_advance_sim<ModelM1>, grid, block, 0, h->stream, h->ptrs, plant->T, plant->num_steps, sigma, seed, h->opt.noise_mask, h->opt.instance_offset);
        break;
    case USVMPC_MODEL_PF_CA:
        hipLaunchKernelGGL(usv_advance_sim<ModelM2>, grid, block, 0, h->stream, h->ptrs, plant->T, plant->num_steps, sigma, seed, h->opt.noise_mask, h->opt.instance_offset);
        break;
#endif
#ifdef USV_GEN_MODEL_HEADER
    case USVMPC_MODEL_GENERATED:
        hipLaunchKernelGGL(usv_advance_sim<ModelGen>, grid, block, 0, h->stream, h->ptrs, plant->T, plant->num_steps, sigma, seed, h->opt.noise_mask, h->opt.instance_offset);
        break;
#endif
    default: h->err = "advance_sim: no plant kernel for this model in this library"; return USVMPC_E_ARG;
    }
    HIP_TRY(h, hipGetLastError());
    h->world.plan_handed_over();
    if (h->opt.tracks_on && h->opt.step_on_advance) return tracks_step(h, plant->T); // (the world moves by the plant's period)
    if (h->world.steps_on_advance(h->opt.step_on_advance != 0)) return world_step(h, plant->T);
    return 0;
}

// ---- the options: option_plan.hpp holds the table (names, checks, normalisation, where a value goes, what it invalidates) and judges a call
// as far as the handle's sizes allow; here: the preconditions on other handle state, the store, the effects and the hooks
static OptFacts option_facts(const usvmpc_handle *h)
{
    return OptFacts{h->N, h->nx, h->nu, h->K, model_has_pairs(h->desc.model), h->spec.any_bsoft != 0, h->spec.boxpack_ok != 0};
}

static int upload_spec(usvmpc_handle *h)
{
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(h->d_spec, &h->spec, sizeof(DevSpec), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

// FX_HOOK, before anything is done: what other state of the handle forbids (nullptr: nothing)
static const char *option_refused(const usvmpc_handle *h, OptId id, double v)
{
    switch (id) {
    case OPT_OBSTACLE_TRACKS: { // (off: p stays as it stands and is the caller's again)
        if (v == 0.0) break;
        const bool pf = h->desc.model == USVMPC_MODEL_PF_CA; // (whose world h->world is)
        if (pf && h->world.fleet_S()) return "obstacle_tracks: a fleet is on (usvmpc_pf_fleet) and the path-following front end owns p on this handle";
        if (!h->tracks_pos_set) return "obstacle_tracks: set \"obs_pos\" before switching the option on";
        if (h->pf_ready) return "obstacle_tracks: the path-following front end owns p on this handle";
        if (pf && h->world.moving()) return "obstacle_tracks: the path-following front end's world moves (usvmpc_pf_world_vel) and owns p on this handle";
        if (!pf && h->world.moving()) return "obstacle_tracks: the guidance front end's world moves (usvmpc_guidance_world_vel) and owns p on this handle";
        break;
    }
    case OPT_HOST_MIRROR:
        if (v != 0.0 && !h->mirror) return "host_mirror cannot be switched on again";
        break;
    default: break;
    }
    return nullptr;
}

// FX_HOOK, after the store
static int option_hook(usvmpc_handle *h, OptId id, double v)
{
    switch (id) {
    case OPT_OBSTACLE_TRACKS:
        if (v != 0.0) h->tracks_dirty = true;
        break;
    case OPT_PF_PREDICT: return h->pf_ready ? apply_static(h) : 0;
    case OPT_SORT_BY_DIFFICULTY:
        if (v == 0.0 && h->ptrs.perm) { h->ptrs.perm = nullptr; h->map_changed = true; }
        break;
    case OPT_KEEP_MULTIPLIERS: { // create the "lam" / "t" buffers now (a partially condensed solve fills them only if they exist)
        DevPtrs &P = h->ptrs;
        if (v == 0.0 || P.lam_out) break;
        HIP_TRY(h, hipSetDevice(h->device));
        P.nlam = lam_len(h->spec, h->soft);
        const size_t cnt = (size_t)h->B * (h->N + 1) * (size_t)(P.nlam > 0 ? P.nlam : 1);
        if (dev_alloc(h, &P.lam_out, cnt, false)) return USVMPC_E_HIP;
        if (dev_alloc(h, &P.t_out, cnt, false)) { P.lam_out = nullptr; return USVMPC_E_HIP; }
        h->export_at = -1;
        break;
    }
    case OPT_HOST_MIRROR: { // 0: drop the pinned host mirror of the caller-visible arrays (every set / get then goes to the device)
        if (v != 0.0 || !h->mirror) break;
        HIP_TRY(h, hipSetDevice(h->device));
        const int rcf = mirror_flush(h);
        if (rcf) return rcf;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->hm.dropped();
        (void)hipHostFree(h->mirror);
        h->mirror = nullptr;
        break;
    }
    default: break;
    }
    return 0;
}

// an accepted value (parse_option's) takes effect: the steps in this order for every option, each where the row asks for it.  Also the
// typed way in for the library's own switches ("static_obstacles": apply_static).
static int apply_option(usvmpc_handle *h, OptId id, double v)
{
    const OptRow &row = OPTION_TABLE[id];
    if (!(row.fx & FX_KEEPS_AHEAD)) { // (options change maps, layouts or launches: a lineariser that ran ahead is not trusted across them)
        const int rcs = spec_cancel(h);
        if (rcs) return rcs;
    }
    const bool act = !(row.fx & FX_IF_CHANGED) || load(h->opt, row.at) != v;
    DevSpec &S = h->spec;
    switch (id) { // the store: Options, or DevSpec for what the kernels read
    case OPT_STATIC_OBSTACLES: S.p_static = v != 0.0; break;
    case OPT_PACK_BOX_ROWS: S.boxpack = v != 0.0; break;
    case OPT_COND_PRED_CORR: S.cpc = v != 0.0; break;
    case OPT_CPC_FACTOR: S.cpc_factor = v; break;
    case OPT_HPIPM_MODE: {
        usvmpc_desc d;
        hpipm_profile(d, (int)v);
        S.mu0 = d.mu0; S.alpha_min = d.alpha_min; S.cpc = d.cond_pred_corr; S.cpc_factor = d.cpc_factor;
        break;
    }
    default: store(h->opt, row.at, v);
    }
    if (act) {
        if (row.fx & FX_CAPS) h->caps.reset();
        if (row.fx & FX_COND_RELEASE) cond_release(h);
        if (row.fx & FX_MAP_CHANGED) h->map_changed = true;
        if (row.fx & FX_LAYOUT_DIRTY) h->layout_dirty = true;
        if (row.fx & FX_TRACKS_DIRTY) h->tracks_dirty = true;
        if (row.fx & FX_UPLOAD_SPEC) {
            const int rcu = upload_spec(h);
            if (rcu) return rcu;
        }
    }
    return (row.fx & FX_HOOK) ? option_hook(h, id, v) : 0;
}

int usvmpc_set_option(usvmpc_handle *h, const char *name, double value)
{
    if (!h) return USVMPC_E_ARG;
    const OptParse p = parse_option(name, value, option_facts(h));
    if (p.rc) { h->err = p.err; return p.rc; }
    if (p.row->fx & FX_HOOK)
        if (const char *why = option_refused(h, p.row->id, p.value)) { h->err = why; return USVMPC_E_ARG; }
    return apply_option(h, p.row->id, p.value);
}


// ---- the front ends' resident world (include/usvmpc.h: usvmpc_guidance_world .. _fleet_state, usvmpc_pf_world .. _fleet_state): world_plan.hpp
// judges a call and says what is to be done; here it is done.  Set-up calls all, a world step apart: they wait for the stream.
static const WorldKind &world_kind(const usvmpc_handle *h) { return h->desc.model == USVMPC_MODEL_PF_CA ? WORLD_PF : WORLD_GUIDANCE; } // (whose world h->world is)

static WorldFacts world_facts(const usvmpc_handle *h, const WorldKind &k)
{
    const bool pf = &k == &WORLD_PF;
    return WorldFacts{&k, h->B, h->desc.model == (pf ? USVMPC_MODEL_PF_CA : USVMPC_MODEL_GUIDANCE_CA1), pf ? h->pf_ready : h->gd_ready,
                      h->opt.tracks_on != 0, h->opt.pf_predict != 0};
}

// "static_obstacles" as the front end needs it: off only while its world moves AND is predicted per stage (a prepare then writes all stages)
static int apply_static(usvmpc_handle *h)
{
    const bool want = h->world.want_static(world_kind(h), h->opt.pf_predict != 0);
    if ((h->spec.p_static != 0) == want) return 0;
    return apply_option(h, OPT_STATIC_OBSTACLES, want ? 1.0 : 0.0);
}

static int pf_alloc(usvmpc_handle *h);
static size_t slots_k(const usvmpc_handle *h) { return (size_t)h->B * (size_t)h->K; } // (instance, slot) pairs

// a world buffer (the list, or the velocities) of `need` doubles in place of the present one, which is released first; the plan hears of both
static int world_buffer(usvmpc_handle *h, double **buf, size_t need, bool vel)
{
    dev_free(h, *buf, (vel ? h->world.vel_cap() : h->world.list_cap()) * sizeof(double));
    *buf = nullptr;
    vel ? h->world.vel_buffer(0, false) : h->world.list_buffer(0);
    if (dev_alloc(h, buf, need, false)) return USVMPC_E_HIP;
    vel ? h->world.vel_buffer(need, true) : h->world.list_buffer(need);
    return 0;
}

// what a judged call does on the device.  in: the caller's list or velocities; out, out2: where a read or a fleet_state answers
static int carry_world(usvmpc_handle *h, const WorldAct &a, const double *in, double T, double *out, void *out2)
{
    usvmpc_handle::WorldBufs &D = h->wb;
    const size_t B = h->B, n = B * (size_t)a.n;
    if (a.what == WORLD_NOTHING) return 0;
    if (a.what == WORLD_FLEET_STATE && a.host_answer) {
        if (out) std::fill(out, out + B, 1e300);
        if (out2) std::fill((int *)out2, (int *)out2 + B, -1);
        return 0;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    if (a.make_front_end) {
        const int rc = pf_alloc(h);
        if (rc) return rc;
    }
    const size_t slots = B * (size_t)(h->K ? h->K : 1);
    if (a.make_tracks && !D.trk_pv && (dev_alloc(h, &D.trk_pv, slots * 4, true) || dev_alloc(h, &D.trk_lh, slots, true))) return USVMPC_E_HIP;
    if (a.make_sep && !D.min_sep) {
        if (dev_alloc(h, &D.min_sep, B, true) || dev_alloc(h, &D.sep_tick, B, true)) return USVMPC_E_HIP;
        hipLaunchKernelGGL(usv_guidance_none_yet, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, D.min_sep, D.sep_tick, (int)B);
        HIP_TRY(h, hipGetLastError());
    }
    if (a.make_plans && !D.chosen) {
        if (dev_alloc(h, &D.chosen, slots, true) || dev_alloc(h, &D.source, slots, true) || dev_alloc(h, &D.plan_fed, 1, true)) return USVMPC_E_HIP;
        HIP_TRY(h, hipMemsetAsync(D.chosen, 0xff, slots * sizeof(int), h->stream)); // (-1)
        HIP_TRY(h, hipMemsetAsync(D.source, 0xff, slots * sizeof(int), h->stream));
        HIP_TRY(h, hipMemsetAsync(D.plan_fed, 0, sizeof(unsigned long long), h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->plan_source_clear = true;
    }
    switch (a.what) {
    case WORLD_UPLOAD_LIST:
    case WORLD_UPLOAD_VEL: {
        const bool vel = a.what == WORLD_UPLOAD_VEL;
        HIP_TRY(h, hipStreamSynchronize(h->stream)); // (a prepare or a world step that reads the old ones may be in flight)
        if (a.grow && world_buffer(h, vel ? &D.vel : &D.list, a.need, vel)) return USVMPC_E_HIP;
        if (a.need) HIP_TRY(h, hipMemcpyAsync(vel ? D.vel : D.list, in, a.need * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return 0;
    }
    case WORLD_RELAYOUT: { // the list laid out anew through the host (fleet_world.hpp: fleet_relayout, which says what is kept; in: the new fixed
        // entries [B][n1_fixed][3]).  Afterwards the list has velocities, whether the world moved before or not.
        const double *fixed = a.new_fixed ? in : nullptr;
        const bool moving = h->world.moving();
        const int n0 = a.n0, n1 = a.n1_fixed + a.f1;
        HIP_TRY(h, hipStreamSynchronize(h->stream)); // (a prepare or a world step on the old list may be in flight)
        std::vector<double> w0(B * (size_t)n0 * 3), v0(B * (size_t)n0 * 2), w1(a.need), v1(a.need_vel);
        if (!w0.empty()) HIP_TRY(h, hipMemcpyAsync(w0.data(), D.list, w0.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (!v0.empty() && moving) HIP_TRY(h, hipMemcpyAsync(v0.data(), D.vel, v0.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t b = 0; b < B; b++)
            fleet_relayout(w0.data() + b * (size_t)n0 * 3, moving ? v0.data() + b * (size_t)n0 * 2 : nullptr, n0 - a.f0, a.f0,
                           fixed ? fixed + b * (size_t)a.n1_fixed * 3 : nullptr, a.n1_fixed, a.f1, w1.data() + b * (size_t)n1 * 3, v1.data() + b * (size_t)n1 * 2);
        if (a.grow && world_buffer(h, &D.list, a.need, false)) return USVMPC_E_HIP;
        if (a.grow_vel && world_buffer(h, &D.vel, a.need_vel, true)) return USVMPC_E_HIP;
        if (!w1.empty()) HIP_TRY(h, hipMemcpyAsync(D.list, w1.data(), w1.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (!v1.empty()) HIP_TRY(h, hipMemcpyAsync(D.vel, v1.data(), v1.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return 0;
    }
    case WORLD_MERGE_VEL: { // [B][nvel][2] into the head of every instance's [n][2]
        const size_t row = (size_t)a.n * 2, head = (size_t)a.nvel * 2;
        std::vector<double> v(B * row);
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipMemcpyAsync(v.data(), D.vel, v.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t b = 0; b < B; b++) std::copy(in + b * head, in + (b + 1) * head, v.begin() + (long)(b * row));
        HIP_TRY(h, hipMemcpyAsync(D.vel, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return 0;
    }
    case WORLD_STEP: // (one kernel for both front ends' worlds: pos += T vel per entry, track_step; no wait - it is part of a tick)
        hipLaunchKernelGGL(usv_pf_world_step, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, D.list, (const double *)D.vel, (long)n, T);
        HIP_TRY(h, hipGetLastError());
        return 0;
    case WORLD_READ: {
        double *vel = (double *)out2;
        if (out && n) HIP_TRY(h, hipMemcpyAsync(out, D.list, n * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (vel && n && a.vel_on_device) HIP_TRY(h, hipMemcpyAsync(vel, D.vel, n * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (vel && !a.vel_on_device) std::fill(vel, vel + n * 2, 0.0); // (a world at rest)
        return 0;
    }
    case WORLD_PLAN_STATE: { // out2: {int *source, long long *fed}
        void **o = (void **)out2;
        if (a.host_answer) {
            if (o[0]) std::fill((int *)o[0], (int *)o[0] + slots_k(h), -1);
            if (o[1]) *(long long *)o[1] = 0;
            return 0;
        }
        if (o[0] && slots_k(h)) HIP_TRY(h, hipMemcpyAsync(o[0], D.source, slots_k(h) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        if (o[1]) HIP_TRY(h, hipMemcpyAsync(o[1], D.plan_fed, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return 0;
    }
    case WORLD_FLEET_STATE:
        if (out) HIP_TRY(h, hipMemcpyAsync(out, D.min_sep, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (out2) HIP_TRY(h, hipMemcpyAsync(out2, D.sep_tick, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return 0;
    default: return 0;
    }
}

// an entry point after its null check: the judged call is refused, or carried out and then made to stand
static int world_call(usvmpc_handle *h, const WorldAct &a, const double *in = nullptr, double T = 0.0, double *out = nullptr, void *out2 = nullptr)
{
    if (!a.refused.empty()) { h->err = a.refused; return USVMPC_E_ARG; }
    const int rc = carry_world(h, a, in, T, out, out2);
    if (rc) return rc;
    h->world.commit(a);
    return a.apply_static ? apply_static(h) : 0;
}

int usvmpc_guidance_world(usvmpc_handle *h, const double *world, int n_world, double max_radius)
{
    return h ? world_call(h, h->world.world(world_facts(h, WORLD_GUIDANCE), world, n_world, max_radius), world) : USVMPC_E_ARG;
}

int usvmpc_pf_world(usvmpc_handle *h, const double *world, int n_world, double max_radius)
{
    return h ? world_call(h, h->world.world(world_facts(h, WORLD_PF), world, n_world, max_radius), world) : USVMPC_E_ARG;
}

int usvmpc_guidance_world_vel(usvmpc_handle *h, const double *vel, int predict)
{
    return h ? world_call(h, h->world.vel(world_facts(h, WORLD_GUIDANCE), vel, predict), vel) : USVMPC_E_ARG;
}

int usvmpc_pf_world_vel(usvmpc_handle *h, const double *vel)
{
    return h ? world_call(h, h->world.vel(world_facts(h, WORLD_PF), vel, 0), vel) : USVMPC_E_ARG;
}

int usvmpc_guidance_world_step(usvmpc_handle *h, double T)
{
    return h ? world_call(h, h->world.step(world_facts(h, WORLD_GUIDANCE), T), nullptr, T) : USVMPC_E_ARG;
}

int usvmpc_pf_world_step(usvmpc_handle *h, double T)
{
    return h ? world_call(h, h->world.step(world_facts(h, WORLD_PF), T), nullptr, T) : USVMPC_E_ARG;
}

// usvmpc_advance, _advance_sim and the cascade's hand-over: the world of the handle's own front end moves with the vessel
static int world_step(usvmpc_handle *h, double T)
{
    return world_call(h, h->world.step(world_facts(h, world_kind(h)), T), nullptr, T);
}

int usvmpc_guidance_world_read(usvmpc_handle *h, double *world, double *vel)
{
    return h ? world_call(h, h->world.read(world_facts(h, WORLD_GUIDANCE)), nullptr, 0.0, world, vel) : USVMPC_E_ARG;
}

int usvmpc_pf_world_read(usvmpc_handle *h, double *world, double *vel)
{
    return h ? world_call(h, h->world.read(world_facts(h, WORLD_PF)), nullptr, 0.0, world, vel) : USVMPC_E_ARG;
}

int usvmpc_guidance_fleet(usvmpc_handle *h, int scene_size, double radius)
{
    return h ? world_call(h, h->world.fleet(world_facts(h, WORLD_GUIDANCE), scene_size, radius)) : USVMPC_E_ARG;
}

int usvmpc_pf_fleet(usvmpc_handle *h, int scene_size, double radius)
{
    return h ? world_call(h, h->world.fleet(world_facts(h, WORLD_PF), scene_size, radius)) : USVMPC_E_ARG;
}

int usvmpc_guidance_fleet_state(usvmpc_handle *h, double *min_separation, int *separation_tick)
{
    return h ? world_call(h, h->world.fleet_state(world_facts(h, WORLD_GUIDANCE)), nullptr, 0.0, min_separation, separation_tick) : USVMPC_E_ARG;
}

int usvmpc_pf_fleet_state(usvmpc_handle *h, double *min_separation, int *separation_tick)
{
    return h ? world_call(h, h->world.fleet_state(world_facts(h, WORLD_PF)), nullptr, 0.0, min_separation, separation_tick) : USVMPC_E_ARG;
}

int usvmpc_guidance_fleet_plans(usvmpc_handle *h, int on)
{
    return h ? world_call(h, h->world.plans(world_facts(h, WORLD_GUIDANCE), on, h->N)) : USVMPC_E_ARG;
}

int usvmpc_pf_fleet_plans(usvmpc_handle *h, int on)
{
    return h ? world_call(h, h->world.plans(world_facts(h, WORLD_PF), on, h->N)) : USVMPC_E_ARG;
}

static int fleet_plan_state(usvmpc_handle *h, const WorldKind &k, int *source, long long *plan_fed, long long *plan_launches)
{
    void *out[2] = {source, plan_fed};
    const int rc = world_call(h, h->world.fleet_plan_state(world_facts(h, k)), nullptr, 0.0, nullptr, out);
    if (rc == 0 && plan_launches) *plan_launches = h->plan_launches;
    return rc;
}

int usvmpc_guidance_fleet_plan_state(usvmpc_handle *h, int *source, long long *plan_fed, long long *plan_launches)
{
    return h ? fleet_plan_state(h, WORLD_GUIDANCE, source, plan_fed, plan_launches) : USVMPC_E_ARG;
}

int usvmpc_pf_fleet_plan_state(usvmpc_handle *h, int *source, long long *plan_fed, long long *plan_launches)
{
    return h ? fleet_plan_state(h, WORLD_PF, source, plan_fed, plan_launches) : USVMPC_E_ARG;
}

// a predicted prepare's last step while plans are on (world_plan.hpp: records_choice): the plan kernel behind the prepare when the iterate
// is one hand-over old, else the sources say "none".  Same stream, no wait.
static int fleet_plans_follow(usvmpc_handle *h, const WorldKind &k, void (*kernel)(FleetPlanArgs), const int *finish_tick)
{
    usvmpc_handle::WorldBufs &D = h->wb;
    const WorldPlan &w = h->world;
    if (!D.source || h->K == 0) return 0; // (plans were never on)
    if (!w.plan_usable(k, h->opt.pf_predict != 0)) { // the sources of the LAST prepare: none, plans on or off
        if (!h->plan_source_clear) HIP_TRY(h, hipMemsetAsync(D.source, 0xff, slots_k(h) * sizeof(int), h->stream)); // (-1)
        h->plan_source_clear = true;
        return 0;
    }
    h->plan_source_clear = false;
    FleetPlanArgs A = {h->ptrs.x, h->ptrs.status, finish_tick, D.chosen, D.trk_pv, const_cast<double *>(h->ptrs.p), D.source, D.plan_fed,
                       h->B, h->N, h->K, w.fleet_S(), w.nfixed()};
    hipLaunchKernelGGL(kernel, dim3((unsigned)((h->B + PLAN_GROUP - 1) / PLAN_GROUP)), dim3(256), 0, h->stream, A);
    HIP_TRY(h, hipGetLastError());
    h->plan_launches++;
    h->world.plan_used();
    return 0;
}

// ---- guidance front end (M1 only): see ca_guidance.hpp (the arithmetic), guidance.hpp (the host-fed kernels), usv_guidance_tick above

static int guidance_alloc(usvmpc_handle *h, int npts)
{
    if (h->desc.model != USVMPC_MODEL_GUIDANCE_CA1) { h->err = "the guidance front end belongs to usv_model_guidance_ca1"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t B = h->B;
    GuidancePtrs &G = h->gd;
    if (!h->gd_ready) {
        double *d; int *i; float *f;
        if (dev_alloc(h, &d, B * 2, true)) return USVMPC_E_HIP; G.vel = d;
        if (dev_alloc(h, &d, B * 3, true)) return USVMPC_E_HIP; G.pose = d;
        if (dev_alloc(h, &d, B * GUIDANCE_LMAX * 3, true)) return USVMPC_E_HIP; G.obs = d;
        if (dev_alloc(h, &i, B, true)) return USVMPC_E_HIP; G.nobs = i;
        if (dev_alloc(h, &G.k, B, true)) return USVMPC_E_HIP;
        if (dev_alloc(h, &f, B, true)) return USVMPC_E_HIP; G.past_psied = f;
        if (dev_alloc(h, &G.ak, B, true)) return USVMPC_E_HIP;
        if (dev_alloc(h, &G.ye, B, true)) return USVMPC_E_HIP;
        if (dev_alloc(h, &G.active, B, true)) return USVMPC_E_HIP;
        if (dev_alloc(h, &G.heading, B, true)) return USVMPC_E_HIP;
        if (dev_alloc(h, &G.rdes, B, true)) return USVMPC_E_HIP;
        if (dev_alloc(h, &G.speed, B, true)) return USVMPC_E_HIP;
        if (dev_alloc(h, &h->gd_psi, B, true)) return USVMPC_E_HIP;
        if (dev_alloc(h, &h->gd_tickp.min_clear, B, true)) return USVMPC_E_HIP;
        if (dev_alloc(h, &h->gd_tickp.finish_tick, B, true)) return USVMPC_E_HIP;
        G.lmax = GUIDANCE_LMAX;
        h->gd_ready = true;
    }
    if (npts > h->gd_npts_cap) { // grow: the old list is released, its slot in the allocation table with it
        dev_free(h, const_cast<double *>(G.wp), B * 2 * (size_t)h->gd_npts_cap * sizeof(double));
        double *d;
        if (dev_alloc(h, &d, B * 2 * (size_t)npts, true)) return USVMPC_E_HIP;
        G.wp = d;
        h->gd_npts_cap = npts;
    }
    return 0;
}

int usvmpc_guidance_reset(usvmpc_handle *h, const double *waypoints, int npts, const double *psi)
{
    if (!h || !waypoints || !psi || npts < 2) return USVMPC_E_ARG;
    int rc = guidance_alloc(h, npts);
    if (rc) return rc;
    GuidancePtrs &G = h->gd;
    G.npts = npts;
    const size_t B = h->B;
    HIP_TRY(h, hipMemcpyAsync(const_cast<double *>(G.wp), waypoints, B * 2 * npts * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->gd_psi, psi, B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(usv_guidance_reset, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, G, h->gd_psi, (int)B);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(usv_guidance_none_yet, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, h->gd_tickp.min_clear,
                       h->gd_tickp.finish_tick, (int)B);
    HIP_TRY(h, hipGetLastError());
    if (h->wb.min_sep) { // (a fleet has been on)
        hipLaunchKernelGGL(usv_guidance_none_yet, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, h->wb.min_sep, h->wb.sep_tick, (int)B);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->gd_tick = 0;
    h->world.plan_lost();
    return apply_static(h);
}

static int guidance_tick(usvmpc_handle *h);

int usvmpc_guidance_prepare(usvmpc_handle *h, const double *vel_uv, const double *pose, const double *obstacles,
                            const int *n_obstacles, int lmax)
{
    // n_obstacles == NULL: keep the body-frame lists usvmpc_guidance_sense left on the device
    if (!h) return USVMPC_E_ARG;
    if ((vel_uv == nullptr) != (pose == nullptr)) { h->err = "guidance_prepare: give both vel_uv and pose, or neither (device-resident)"; return USVMPC_E_ARG; }
    if (lmax < 0 || lmax > GUIDANCE_LMAX) return USVMPC_E_ARG;
    if (!h->gd_ready || h->gd.npts < 2) { h->err = "usvmpc_guidance_reset must be called first"; return USVMPC_E_ARG; }
    if (!vel_uv) return guidance_tick(h);
    if (h->world.fleet_S()) {
        h->err = "guidance_prepare: a fleet is on and its scene exists on the device only; prepare device-resident (vel_uv and pose NULL)";
        return USVMPC_E_ARG;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    {
        const int rcf = mirror_flush(h);
        if (rcf) return rcf;
    }
    GuidancePtrs &G = h->gd;
    const size_t B = h->B;
    HIP_TRY(h, hipMemcpyAsync(const_cast<double *>(G.vel), vel_uv, B * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(const_cast<double *>(G.pose), pose, B * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (n_obstacles)
        HIP_TRY(h, hipMemcpyAsync(const_cast<int *>(G.nobs), n_obstacles, B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (n_obstacles && lmax > 0) {
        if (!obstacles) return USVMPC_E_ARG;
        // [B][lmax][3] -> [B][GUIDANCE_LMAX][3]
        HIP_TRY(h, hipMemcpy2DAsync(const_cast<double *>(G.obs), GUIDANCE_LMAX * 3 * sizeof(double), obstacles,
                                    (size_t)lmax * 3 * sizeof(double), (size_t)lmax * 3 * sizeof(double), B,
                                    hipMemcpyHostToDevice, h->stream));
    }
    hipLaunchKernelGGL(usv_guidance_pre, dim3((unsigned)((B + GUIDANCE_BLOCK - 1) / GUIDANCE_BLOCK)), dim3(GUIDANCE_BLOCK), 0, h->stream, h->ptrs, G);
    HIP_TRY(h, hipGetLastError());
    // the copies above read caller memory: it must be reusable when this call returns (pinned buffers make
    // hipMemcpyAsync truly asynchronous)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

// the device-resident tick (usvmpc_guidance_prepare with vel_uv and pose NULL): ONE launch on the handle's stream, no synchronisation.  It
// writes x0, p and lh only - nothing a lineariser reads - so a linearisation made a tick ahead stands (no spec_cancel, unlike usvmpc_pf_prepare).
static int guidance_tick(usvmpc_handle *h)
{
    if (!h->world.exists()) { h->err = "guidance_prepare: the device-resident tick needs a world list (usvmpc_guidance_world first; an empty one will do)"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    const int rcf = mirror_flush(h);
    if (rcf) return rcf;
    const WorldPlan &w = h->world;
    const usvmpc_handle::WorldBufs &D = h->wb;
    CaTickPtrs W = h->gd_tickp;
    W.world = D.list; W.nworld = w.nworld(); W.max_radius = w.max_radius();
    W.trk_pv = D.trk_pv; W.trk_lh = D.trk_lh;
    W.wvel = w.want_static(WORLD_GUIDANCE, false) ? nullptr : D.vel; // (held still inside the horizon: the tick of a world at rest)
    W.tick = h->gd_tick;
    W.chosen = w.records_choice(WORLD_GUIDANCE, false) ? D.chosen : nullptr;
    const size_t B = h->B;
    if (w.fleet_S()) { // the scene's other vessels, as the plant left them, into the fleet slots - before usv_guidance_tick rewrites x0
        const long n = (long)B * fleet_slots(w.fleet_S());
        hipLaunchKernelGGL(usv_guidance_fleet_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->ptrs.x0, D.list, D.vel,
                           D.min_sep, D.sep_tick, (long)B, w.fleet_S(), w.nfixed(), w.fleet_radius(), h->gd_tick);
        HIP_TRY(h, hipGetLastError());
    }
    hipLaunchKernelGGL(usv_guidance_tick, dim3((unsigned)((B + CA_GROUP - 1) / CA_GROUP)), dim3(256), 0, h->stream, h->ptrs, h->gd, W);
    HIP_TRY(h, hipGetLastError());
    h->gd_tick++;
    return fleet_plans_follow(h, WORLD_GUIDANCE, usv_guidance_fleet_plans, W.finish_tick);
}

int usvmpc_guidance_sense(usvmpc_handle *h, const double *pose, const double *world, int n_world, double max_radius,
                          double *obstacles, int *n_obstacles)
{
    if (!h || !pose || n_world < 0 || (n_world > 0 && !world)) return USVMPC_E_ARG;
    if (!h->gd_ready) { h->err = "usvmpc_guidance_reset must be called first"; return USVMPC_E_ARG; }
    if (h->world.fleet_S()) {
        h->err = "guidance_sense: a fleet is on and its scene exists on the device only; prepare device-resident (usvmpc_guidance_prepare, vel_uv and pose NULL)";
        return USVMPC_E_ARG;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    GuidancePtrs &G = h->gd;
    const size_t B = h->B;
    if ((size_t)n_world > h->gd_sense_world_cap) {
        dev_free(h, h->gd_sense_world, B * h->gd_sense_world_cap * 3 * sizeof(double));
        h->gd_sense_world = nullptr;
        if (dev_alloc(h, &h->gd_sense_world, B * (size_t)n_world * 3, true)) return USVMPC_E_HIP;
        h->gd_sense_world_cap = (size_t)n_world;
    }
    HIP_TRY(h, hipMemcpyAsync(const_cast<double *>(G.pose), pose, B * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (n_world > 0)
        HIP_TRY(h, hipMemcpyAsync(h->gd_sense_world, world, B * (size_t)n_world * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(usv_obstacle_sim, dim3((unsigned)((B + 127) / 128)), dim3(128), 0, h->stream, G, h->gd_sense_world, n_world,
                       max_radius, (int)B);
    HIP_TRY(h, hipGetLastError());
    if (obstacles)
        HIP_TRY(h, hipMemcpyAsync(obstacles, G.obs, B * GUIDANCE_LMAX * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (n_obstacles)
        HIP_TRY(h, hipMemcpyAsync(n_obstacles, G.nobs, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (obstacles || n_obstacles) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int usvmpc_guidance_publish(usvmpc_handle *h, double *heading, double *r_des, double *speed, double *ye, int *active)
{
    if (!h) return USVMPC_E_ARG;
    if (!h->gd_ready) { h->err = "usvmpc_guidance_reset must be called first"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    GuidancePtrs &G = h->gd;
    const size_t B = h->B;
    hipLaunchKernelGGL(usv_guidance_post, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, h->ptrs, G);
    HIP_TRY(h, hipGetLastError());
    if (heading) HIP_TRY(h, hipMemcpyAsync(heading, G.heading, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (r_des) HIP_TRY(h, hipMemcpyAsync(r_des, G.rdes, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (speed) HIP_TRY(h, hipMemcpyAsync(speed, G.speed, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (ye) HIP_TRY(h, hipMemcpyAsync(ye, G.ye, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (active) HIP_TRY(h, hipMemcpyAsync(active, G.active, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (heading || r_des || speed || ye || active) HIP_TRY(h, hipStreamSynchronize(h->stream)); // (every output NULL: enqueued only)
    return 0;
}

int usvmpc_guidance_state(usvmpc_handle *h, int *wp_index, float *past_psied)
{
    if (!h) return USVMPC_E_ARG;
    if (!h->gd_ready) { h->err = "usvmpc_guidance_reset must be called first"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t B = h->B;
    if (wp_index) HIP_TRY(h, hipMemcpyAsync(wp_index, h->gd.k, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (past_psied) HIP_TRY(h, hipMemcpyAsync(past_psied, h->gd.past_psied, B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ---- the guidance front end's mission state (include/usvmpc.h; its resident world: carry_world above)
static int gd_check(usvmpc_handle *h, const char *who)
{
    if (h->desc.model != USVMPC_MODEL_GUIDANCE_CA1) { h->err = std::string(who) + ": the guidance front end belongs to usv_model_guidance_ca1"; return USVMPC_E_ARG; }
    if (!h->gd_ready) { h->err = std::string(who) + ": usvmpc_guidance_reset must be called first"; return USVMPC_E_ARG; }
    return 0;
}

int usvmpc_guidance_mission_state(usvmpc_handle *h, int *wp_index, float *past_psied, int *finish_tick, double *min_clearance)
{
    if (!h) return USVMPC_E_ARG;
    int rc = gd_check(h, "guidance_mission_state");
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t B = h->B;
    if (wp_index) HIP_TRY(h, hipMemcpyAsync(wp_index, h->gd.k, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (past_psied) HIP_TRY(h, hipMemcpyAsync(past_psied, h->gd.past_psied, B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (finish_tick) HIP_TRY(h, hipMemcpyAsync(finish_tick, h->gd_tickp.finish_tick, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (min_clearance) HIP_TRY(h, hipMemcpyAsync(min_clearance, h->gd_tickp.min_clear, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ---- path-following front end (usv_model_pf_ca only): see pf_guidance.hpp
static int pf_check(usvmpc_handle *h)
{
    if (h->desc.model != USVMPC_MODEL_PF_CA) { h->err = "the path-following front end (usvmpc_pf_*) belongs to usv_model_pf_ca"; return USVMPC_E_ARG; }
    return 0;
}

static int pf_alloc(usvmpc_handle *h)
{
    if (h->pf_alloc) return 0;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t B = h->B;
    PfPtrs &F = h->pf;
    if (dev_alloc(h, &F.k, B, true) || dev_alloc(h, &F.phase, B, true) || dev_alloc(h, &F.finish_tick, B, true) || dev_alloc(h, &F.past, B * 2, true) ||
        dev_alloc(h, &F.last, B * 3, true) || dev_alloc(h, &F.u, B, true) || dev_alloc(h, &F.ye, B, true) || dev_alloc(h, &F.min_clear, B, true) ||
        dev_alloc(h, &F.yref_writes, 1, true) || dev_alloc(h, &F.thr_port, B, true) || dev_alloc(h, &F.thr_stbd, B, true) ||
        dev_alloc(h, &F.Tx, B, true) || dev_alloc(h, &F.Tz, B, true) || dev_alloc(h, &F.speed, B, true) || dev_alloc(h, &F.e_u, B, true) ||
        dev_alloc(h, &F.e_ye, B, true) || dev_alloc(h, &F.active, B, true) || dev_alloc(h, &h->pf_vel, B * 3, true) ||
        dev_alloc(h, &h->pf_pose, B * 3, true) || dev_alloc(h, &h->wb.min_sep, B, true) || dev_alloc(h, &h->wb.sep_tick, B, true))
        return USVMPC_E_HIP;
    h->pf_alloc = true;
    return 0;
}

// the front end's kernel arguments: its own buffers and the handle's world (wvel: null, a world at rest, unless the caller says otherwise)
static PfPtrs pf_args(const usvmpc_handle *h)
{
    PfPtrs F = h->pf;
    F.world = h->wb.list; F.nworld = h->world.nworld(); F.max_radius = h->world.max_radius();
    F.trk_pv = h->wb.trk_pv; F.trk_lh = h->wb.trk_lh;
    F.min_sep = h->wb.min_sep; F.sep_tick = h->wb.sep_tick;
    F.chosen = nullptr; // (usvmpc_pf_prepare says otherwise while plans are on)
    return F;
}

int usvmpc_pf_reset(usvmpc_handle *h, const double *waypoints, int npts)
{
    if (!h) return USVMPC_E_ARG;
    int rc = pf_check(h);
    if (rc) return rc;
    if (!waypoints || npts < 2) { h->err = "pf_reset: a waypoint list of at least two points is needed"; return USVMPC_E_ARG; }
    if (h->opt.tracks_on) { h->err = "pf_reset: option \"obstacle_tracks\" is on and the tracks own p; switch it off first"; return USVMPC_E_ARG; }
    rc = pf_alloc(h);
    if (rc) return rc;
    PfPtrs &F = h->pf;
    const size_t B = h->B;
    if (npts > h->pf_npts_cap) {
        dev_free(h, const_cast<double *>(F.wp), B * 2 * (size_t)h->pf_npts_cap * sizeof(double));
        F.wp = nullptr; h->pf_npts_cap = 0;
        double *d = nullptr;
        if (dev_alloc(h, &d, B * 2 * (size_t)npts, true)) return USVMPC_E_HIP;
        F.wp = d;
        h->pf_npts_cap = npts;
    }
    F.npts = npts;
    HIP_TRY(h, hipMemcpyAsync(const_cast<double *>(F.wp), waypoints, B * 2 * (size_t)npts * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(usv_pf_reset, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, pf_args(h), (int)B);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->pf_ready = true; h->pf_stale = true; h->pf_tick = 0;
    h->world.plan_lost();
    return apply_static(h);
}

int usvmpc_pf_prepare(usvmpc_handle *h, const double *vel_uvr, const double *pose)
{
    if (!h) return USVMPC_E_ARG;
    int rc = pf_check(h);
    if (rc) return rc;
    if (!h->pf_ready) { h->err = "usvmpc_pf_reset must be called first"; return USVMPC_E_ARG; }
    if ((vel_uvr == nullptr) != (pose == nullptr)) { h->err = "pf_prepare: give both vel_uvr and pose, or neither (device-resident)"; return USVMPC_E_ARG; }
    const WorldPlan &w = h->world;
    if (vel_uvr && w.fleet_S()) {
        h->err = "pf_prepare: a fleet is on and its scene exists on the device only; prepare device-resident (both NULL)";
        return USVMPC_E_ARG;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    rc = mirror_flush(h);
    if (rc) return rc;
    rc = spec_cancel(h); // (a caller write of yref as far as the pipelined lineariser is concerned: pf_guidance.hpp)
    if (rc) return rc;
    if (w.fleet_S()) { // the scene's other vessels, as the plant left them, into the fleet slots - before usv_pf_prepare rewrites x0[1..3]
        const long n = (long)h->B * fleet_slots(w.fleet_S());
        hipLaunchKernelGGL(usv_pf_fleet_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->ptrs.x0, h->wb.list, h->wb.vel,
                           h->wb.min_sep, h->wb.sep_tick, (long)h->B, w.fleet_S(), w.nfixed(), w.fleet_radius(), h->pf_tick);
        HIP_TRY(h, hipGetLastError());
    }
    PfPtrs F = pf_args(h);
    F.margin = h->opt.pf_margin;
    F.wvel = w.want_static(WORLD_PF, h->opt.pf_predict != 0) ? nullptr : h->wb.vel; // (held still inside the horizon: the prepare of a world at rest)
    F.chosen = w.records_choice(WORLD_PF, h->opt.pf_predict != 0) ? h->wb.chosen : nullptr;
    const size_t B = h->B;
    if (vel_uvr) {
        HIP_TRY(h, hipMemcpyAsync(h->pf_vel, vel_uvr, B * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->pf_pose, pose, B * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        F.vel = h->pf_vel; F.pose = h->pf_pose;
    } else {
        F.vel = nullptr; F.pose = nullptr;
    }
    hipLaunchKernelGGL(usv_pf_prepare, dim3((unsigned)((B + PF_GROUP - 1) / PF_GROUP)), dim3(256), 0, h->stream, h->ptrs, F, h->pf_tick, h->pf_stale ? 1 : 0);
    HIP_TRY(h, hipGetLastError());
    h->pf_stale = false;
    h->pf_tick++;
    if (vel_uvr) HIP_TRY(h, hipStreamSynchronize(h->stream)); // (the copies read caller memory: it must be reusable when this call returns)
    return fleet_plans_follow(h, WORLD_PF, usv_pf_fleet_plans, F.finish_tick);
}

int usvmpc_pf_publish(usvmpc_handle *h, double *thr_port, double *thr_stbd, double *Tx, double *Tz, float *e_u, float *e_ye, double *speed,
                      int *active)
{
    if (!h) return USVMPC_E_ARG;
    int rc = pf_check(h);
    if (rc) return rc;
    if (!h->pf_ready) { h->err = "usvmpc_pf_reset must be called first"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    const PfPtrs F = pf_args(h);
    const size_t B = h->B;
    hipLaunchKernelGGL(usv_pf_publish, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, h->ptrs, F);
    HIP_TRY(h, hipGetLastError());
    if (thr_port) HIP_TRY(h, hipMemcpyAsync(thr_port, F.thr_port, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (thr_stbd) HIP_TRY(h, hipMemcpyAsync(thr_stbd, F.thr_stbd, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (Tx) HIP_TRY(h, hipMemcpyAsync(Tx, F.Tx, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (Tz) HIP_TRY(h, hipMemcpyAsync(Tz, F.Tz, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (e_u) HIP_TRY(h, hipMemcpyAsync(e_u, F.e_u, B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (e_ye) HIP_TRY(h, hipMemcpyAsync(e_ye, F.e_ye, B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (speed) HIP_TRY(h, hipMemcpyAsync(speed, F.speed, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (active) HIP_TRY(h, hipMemcpyAsync(active, F.active, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (thr_port || thr_stbd || Tx || Tz || e_u || e_ye || speed || active) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int usvmpc_pf_state(usvmpc_handle *h, int *wp_index, int *finish_tick, double *min_clearance, long long *yref_writes)
{
    if (!h) return USVMPC_E_ARG;
    int rc = pf_check(h);
    if (rc) return rc;
    if (!h->pf_ready) { h->err = "usvmpc_pf_reset must be called first"; return USVMPC_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    const PfPtrs &F = h->pf;
    const size_t B = h->B;
    if (wp_index) HIP_TRY(h, hipMemcpyAsync(wp_index, F.k, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (finish_tick) HIP_TRY(h, hipMemcpyAsync(finish_tick, F.finish_tick, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (min_clearance) HIP_TRY(h, hipMemcpyAsync(min_clearance, F.min_clear, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (yref_writes) HIP_TRY(h, hipMemcpyAsync(yref_writes, F.yref_writes, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int usvmpc_calibrate_traffic(usvmpc_handle *h, int nplanes, double *bytes_read, double *bytes_written)
{
    if (!h || nplanes < 1) return USVMPC_E_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    {
        const int rcs = spec_cancel(h);
        if (rcs) return rcs;
    }
    const long stride = (long)h->Bp * LANES;
    const long avail = (long)(h->N + 1) * ws_planes(h);
    if (nplanes + 1 > avail) { h->err = "nplanes exceeds the workspace"; return USVMPC_E_ARG; }
    if ((size_t)h->Bp * (size_t)(nplanes + 1) * 128u > (size_t)UINT32_MAX) { // (usv_calib_stream addresses it all through one 32-bit window)
        h->err = "nplanes * batch exceeds the 4 GiB buffer window of the calibration kernel";
        return USVMPC_E_ARG;
    }
    const long groups = h->Bp;
    hipLaunchKernelGGL(usv_calib_stream, dim3((unsigned)((groups * LANES + 63) / 64)), dim3(64), 0, h->stream, h->ptrs, groups, nplanes);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (bytes_read) *bytes_read = (double)nplanes * stride * 8.0;
    if (bytes_written) *bytes_written = (double)stride * 8.0;
    return 0;
}

// ---- the two-layer control stack (include/usvmpc.h, "Cascade"): kernels usv_cascade_refs / usv_cascade_step above, arithmetic cascade.hpp.
// The object owns its buffers (plain hipMalloc: the guidance handle's allocation table and usvmpc_device_bytes are untouched; the log's
// buffers alone come from the guidance handle's dev_alloc, so that usvmpc_device_bytes counts them) and works on the guidance handle's
// stream as it is at each call; the low-level solver is a set of device pointers into another library's handle.
struct usvmpc_cascade {
    usvmpc_handle *g;
    int ratio, num_steps;
    double T, c;
    long long offset;
    long long tick;   // low-level ticks stepped since the last reset
    bool ready;       // usvmpc_cascade_reset has run
    CascadePtrs p;
    double *d_pose, *d_vel; // [B][3] each: staging of usvmpc_cascade_reset
    // The log (usvmpc_cascade_log_*): which tick records, the counters and the layout are cascade_log_plan.hpp's - CasLogPlan, host-only and
    // checked on the CPU by tests/test_cascade_log_plan.py; no field of it is assigned in this file.  Here: the buffers its layout sizes, from
    // the guidance handle's dev_alloc (nullptr: channel not recorded), and the kernel arguments that do not change from tick to tick.
    CasLogPlan log;
    void *log_buf[CAS_LOG_CHANNELS] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    CasLogRec log_rec = {};
    std::string err;
};
thread_local std::string g_cascade_create_err;

#define CAS_TRY(c, call)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (c)->err = std::string(#call) + ": " + hipGetErrorString(e_);                         \
            return USVMPC_E_HIP;                                                                  \
        }                                                                                         \
    } while (0)

static void cascade_free(usvmpc_cascade *c)
{
    CascadePtrs &p = c->p;
    (void)hipFree(p.s); (void)hipFree(p.thr); (void)hipFree(p.past); (void)hipFree(p.last); (void)hipFree(p.ticks); (void)hipFree(p.sums);
    (void)hipFree(p.yref_writes); (void)hipFree(c->d_pose); (void)hipFree(c->d_vel);
}

// ---- the cascade's log: cascade_log_plan.hpp says what a tick does and what a read copies; here: the buffers, the launch, the copies
static void cascade_log_release(usvmpc_cascade *c)
{
    const CasLogLayout &l = c->log.lay;
    const long long have[CAS_LOG_CHANNELS] = {l.state_bytes, l.thrust_bytes, l.ref_bytes, l.err_bytes, l.status_bytes};
    for (int i = 0; i < CAS_LOG_CHANNELS; i++) {
        if (c->log_buf[i]) dev_free(c->g, c->log_buf[i], (size_t)have[i]);
        c->log_buf[i] = nullptr;
    }
}

// a low-level tick of a cascade whose log runs (usvmpc_cascade_step, ahead of usv_cascade_step)
static int cascade_log_tick(usvmpc_cascade *c)
{
    const LogTick t = c->log.on_tick();
    if (t.slot < 0) return 0;
    usvmpc_handle *h = c->g;
    const CasLogLayout &l = c->log.lay;
    CasLogRec r = c->log_rec;
    const long at = (long)t.slot * l.B;
    long n = 0;
    if (c->log_buf[CAS_LOG_STATE]) { r.r_state = (double *)c->log_buf[CAS_LOG_STATE] + at * l.nsel; n = std::max(n, (long)l.B * l.nsel); }
    if (c->log_buf[CAS_LOG_THRUST]) { r.r_thrust = (double *)c->log_buf[CAS_LOG_THRUST] + at * 2; n = std::max(n, (long)l.B * 2); }
    if (c->log_buf[CAS_LOG_REF]) { r.r_ref = (double *)c->log_buf[CAS_LOG_REF] + at * 2; n = std::max(n, (long)l.B * 2); }
    if (c->log_buf[CAS_LOG_ERR]) { r.r_err = (float *)c->log_buf[CAS_LOG_ERR] + at * 2; n = std::max(n, (long)l.B * 2); }
    if (c->log_buf[CAS_LOG_STATUS]) { r.r_status = (int *)c->log_buf[CAS_LOG_STATUS] + at; n = std::max(n, (long)l.B); }
    hipLaunchKernelGGL(usv_cascade_record, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, r);
    CAS_TRY(c, hipGetLastError());
    return 0;
}

int usvmpc_cascade_create(usvmpc_handle *guidance, int ratio, double T, int num_steps, double c, long long instance_offset, int ll_batch,
                          int ll_N, void *ll_x0, void *ll_x, void *ll_yref, void *ll_yref_e, usvmpc_cascade **out)
{
    std::string &err = g_cascade_create_err;
    if (out) *out = nullptr;
    if (!guidance || !out) { err = "usvmpc_cascade_create: null guidance handle or output"; return USVMPC_E_ARG; }
    usvmpc_handle *h = guidance;
    if (h->desc.model != USVMPC_MODEL_GUIDANCE_CA1) { err = "usvmpc_cascade_create: the upper layer must be a usv_model_guidance_ca1 handle"; return USVMPC_E_ARG; }
    if (!h->gd_ready || h->gd.npts < 2) { err = "usvmpc_cascade_create: usvmpc_guidance_reset must be called first"; return USVMPC_E_ARG; }
    if (!h->world.exists()) { err = "usvmpc_cascade_create: the guidance handle needs a world list (usvmpc_guidance_world first; an empty one will do)"; return USVMPC_E_ARG; }
    if (T - T != 0.0 || c - c != 0.0) { err = "usvmpc_cascade_create: T and c must be finite"; return USVMPC_E_ARG; }
    if (ratio < 1 || num_steps < 1 || !(T > 0.0) || instance_offset < 0) { err = "usvmpc_cascade_create: ratio >= 1, num_steps >= 1, T > 0 and instance_offset >= 0 are needed"; return USVMPC_E_ARG; }
    if (fabs((double)ratio * T - h->spec.dt) > 1e-9 * h->spec.dt) {
        err = "usvmpc_cascade_create: ratio * T = " + std::to_string((double)ratio * T) + " differs from the guidance layer's shooting interval " +
              std::to_string(h->spec.dt);
        return USVMPC_E_ARG;
    }
    if (!ll_x0 || !ll_x || !ll_yref || !ll_yref_e) { err = "usvmpc_cascade_create: null device pointer of the low-level solver (x0, x, yref, yref_e)"; return USVMPC_E_ARG; }
    if (ll_N < 1 || ll_batch != h->B) {
        err = "usvmpc_cascade_create: the low-level solver needs ll_N >= 1 and the guidance handle's batch (" + std::to_string(h->B) + "), got ll_N " +
              std::to_string(ll_N) + ", batch " + std::to_string(ll_batch);
        return USVMPC_E_ARG;
    }
    if (((uintptr_t)ll_yref | (uintptr_t)ll_yref_e) & 15u) { err = "usvmpc_cascade_create: yref and yref_e of the low-level solver must be 16-byte aligned"; return USVMPC_E_ARG; }
    usvmpc_cascade *cs = new usvmpc_cascade();
    cs->g = h; cs->ratio = ratio; cs->num_steps = num_steps; cs->T = T; cs->c = c; cs->offset = instance_offset; cs->tick = 0; cs->ready = false;
    cs->p = CascadePtrs{};
    cs->d_pose = cs->d_vel = nullptr;
    cs->p.ll_x0 = (double *)ll_x0; cs->p.ll_x = (const double *)ll_x; cs->p.ll_yref = (double *)ll_yref; cs->p.ll_yref_e = (double *)ll_yref_e;
    cs->p.ll_N = ll_N;
    const size_t B = (size_t)h->B;
    hipError_t e = hipSetDevice(h->device);
    auto get = [&](auto **ptr, size_t n) { if (e == hipSuccess) e = hipMalloc((void **)ptr, n * sizeof(**ptr)); };
    get(&cs->p.s, B * CAS_NS); get(&cs->p.thr, B * 2); get(&cs->p.past, B * 2); get(&cs->p.last, B * 2); get(&cs->p.ticks, B);
    get(&cs->p.sums, B * 4); get(&cs->p.yref_writes, (size_t)1); get(&cs->d_pose, B * 3); get(&cs->d_vel, B * 3);
    if (e != hipSuccess) {
        err = std::string("usvmpc_cascade_create: ") + hipGetErrorString(e);
        cascade_free(cs);
        delete cs;
        return USVMPC_E_HIP;
    }
    *out = cs;
    return 0;
}

int usvmpc_cascade_destroy(usvmpc_cascade *c)
{
    if (!c) return USVMPC_E_ARG;
    (void)hipSetDevice(c->g->device);
    (void)hipStreamSynchronize(c->g->stream);
    if (c->log.on()) { cascade_log_release(c); c->log.stop(); }
    cascade_free(c);
    delete c;
    return 0;
}

int usvmpc_cascade_reset(usvmpc_cascade *c, const double *pose, const double *vel)
{
    if (!c) return USVMPC_E_ARG;
    if (!pose || !vel) { c->err = "cascade_reset: null pose or vel"; return USVMPC_E_ARG; }
    if (c->log.on()) { c->err = "cascade_reset: a log is running (usvmpc_cascade_log_stop first)"; return USVMPC_E_ARG; }
    usvmpc_handle *h = c->g;
    const size_t B = (size_t)h->B;
    for (size_t i = 0; i < 3 * B; i++)
        if (pose[i] - pose[i] != 0.0 || vel[i] - vel[i] != 0.0) { c->err = "cascade_reset: entry " + std::to_string(i) + " of pose or vel is not finite"; return USVMPC_E_ARG; }
    CAS_TRY(c, hipSetDevice(h->device));
    if (mirror_flush(h)) { c->err = "cascade_reset: " + h->err; return USVMPC_E_HIP; } // (a pending host write of the guidance x0 goes up first)
    CAS_TRY(c, hipMemcpyAsync(c->d_pose, pose, 3 * B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CAS_TRY(c, hipMemcpyAsync(c->d_vel, vel, 3 * B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(usv_cascade_reset, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, c->p, (const double *)c->d_pose,
                       (const double *)c->d_vel, const_cast<double *>(h->ptrs.x0), (int)B);
    CAS_TRY(c, hipGetLastError());
    CAS_TRY(c, hipStreamSynchronize(h->stream)); // (the copies read caller memory)
    c->tick = 0;
    c->ready = true;
    return 0;
}

int usvmpc_cascade_refs(usvmpc_cascade *c)
{
    if (!c) return USVMPC_E_ARG;
    if (!c->ready) { c->err = "cascade_refs: usvmpc_cascade_reset must be called first"; return USVMPC_E_ARG; }
    usvmpc_handle *h = c->g;
    CAS_TRY(c, hipSetDevice(h->device));
    hipLaunchKernelGGL(usv_cascade_refs, dim3((unsigned)((h->B + CAS_GROUP - 1) / CAS_GROUP)), dim3(256), 0, h->stream, h->gd, c->p, h->B);
    CAS_TRY(c, hipGetLastError());
    return 0;
}

int usvmpc_cascade_step(usvmpc_cascade *c, double sigma, unsigned long long seed)
{
    if (!c) return USVMPC_E_ARG;
    if (!c->ready) { c->err = "cascade_step: usvmpc_cascade_reset must be called first"; return USVMPC_E_ARG; }
    if (sigma - sigma != 0.0) { c->err = "cascade_step: sigma is not finite"; return USVMPC_E_ARG; }
    usvmpc_handle *h = c->g;
    CAS_TRY(c, hipSetDevice(h->device));
    const bool hand_over = cas_hands_over(c->tick, c->ratio);
    if (hand_over && mirror_flush(h)) { c->err = "cascade_step: " + h->err; return USVMPC_E_HIP; }
    if (c->log.on()) { // (ahead of the kernel that overwrites the vessel's state)
        const int rcl = cascade_log_tick(c);
        if (rcl) return rcl;
    }
    hipLaunchKernelGGL(usv_cascade_step, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, h->stream, c->p, const_cast<double *>(h->ptrs.x0),
                       h->B, c->T, c->num_steps, c->c, sigma, seed, c->offset, hand_over ? 1 : 0);
    CAS_TRY(c, hipGetLastError());
    c->tick++;
    if (hand_over) h->world.plan_handed_over();
    // a guidance period has passed: the guidance layer's moving world follows, as usvmpc_advance would have moved it
    if (hand_over && h->world.steps_on_advance(h->opt.step_on_advance != 0) && world_step(h, (double)c->ratio * c->T)) {
        c->err = "cascade_step: " + h->err;
        return USVMPC_E_HIP;
    }
    return 0;
}

int usvmpc_cascade_state(usvmpc_cascade *c, double *state, double *thrust, double *past_thrust, int *ticks, long long *yref_writes, double *err_sums)
{
    if (!c) return USVMPC_E_ARG;
    if (!c->ready) { c->err = "cascade_state: usvmpc_cascade_reset must be called first"; return USVMPC_E_ARG; }
    usvmpc_handle *h = c->g;
    const size_t B = (size_t)h->B;
    CAS_TRY(c, hipSetDevice(h->device));
    if (state) CAS_TRY(c, hipMemcpyAsync(state, c->p.s, B * CAS_NS * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (thrust) CAS_TRY(c, hipMemcpyAsync(thrust, c->p.thr, B * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (past_thrust) CAS_TRY(c, hipMemcpyAsync(past_thrust, c->p.past, B * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (ticks) CAS_TRY(c, hipMemcpyAsync(ticks, c->p.ticks, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (yref_writes) CAS_TRY(c, hipMemcpyAsync(yref_writes, c->p.yref_writes, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    if (err_sums) CAS_TRY(c, hipMemcpyAsync(err_sums, c->p.sums, B * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CAS_TRY(c, hipStreamSynchronize(h->stream));
    return 0;
}

int usvmpc_cascade_log_start(usvmpc_cascade *c, const usvmpc_cascade_log_desc *d, const int *ll_status, const int *ll_qp_iter)
{
    if (!c) return USVMPC_E_ARG;
    if (!d) { c->err = "cascade_log_start: null descriptor"; return USVMPC_E_ARG; }
    if (c->log.on()) { c->err = "cascade_log_start: a log is running (usvmpc_cascade_log_stop first)"; return USVMPC_E_ARG; }
    usvmpc_handle *h = c->g;
    CasLogDesc ld = {};
    ld.capacity = d->capacity; ld.every = d->every; ld.first = d->first; ld.state_mask = d->state_mask;
    ld.record_thrust = d->record_thrust; ld.record_ref = d->record_ref; ld.record_err = d->record_err; ld.record_status = d->record_status;
    CasLogLayout lay;
    if (const char *why = check_cas_log_desc(ld, h->B, &lay)) { c->err = why; return USVMPC_E_ARG; }
    if (lay.status_bytes && (!ll_status || !ll_qp_iter)) {
        c->err = "cascade_log_start: the status channel needs the low-level solver's device pointers (status, qp_iter)";
        return USVMPC_E_ARG;
    }
    CAS_TRY(c, hipSetDevice(h->device));
    // all five buffers or none: a failed allocation leaves the cascade and the guidance handle's count as they were
    const long long want[CAS_LOG_CHANNELS] = {lay.state_bytes, lay.thrust_bytes, lay.ref_bytes, lay.err_bytes, lay.status_bytes};
    char *buf[CAS_LOG_CHANNELS] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < CAS_LOG_CHANNELS; i++) {
        if (want[i] == 0) continue;
        if (dev_alloc(h, &buf[i], (size_t)want[i], false)) {
            (void)hipGetLastError();
            c->err = "cascade_log_start: allocation of " + std::to_string(want[i]) + " bytes: " + h->err;
            for (int j = 0; j < i; j++) dev_free(h, buf[j], (size_t)want[j]);
            return USVMPC_E_HIP;
        }
    }
    for (int i = 0; i < CAS_LOG_CHANNELS; i++) c->log_buf[i] = buf[i];
    c->log.start(ld, lay);
    CasLogRec r = {};
    r.s = c->p.s; r.last = c->p.last; r.ll_x = c->p.ll_x;
    r.ll_status = ll_status; r.ll_qp_iter = ll_qp_iter;
    r.g_status = h->ptrs.status; r.g_qp_iter = h->ptrs.qp_iter;
    r.B = h->B; r.ll_N = c->p.ll_N;
    int nsel = 0;
    r.sel = log_pack_mask(ld.state_mask, &nsel);
    r.nsel = nsel;
    c->log_rec = r;
    return 0;
}

int usvmpc_cascade_log_stop(usvmpc_cascade *c)
{
    if (!c) return USVMPC_E_ARG;
    if (!c->log.on()) { c->err = "cascade_log_stop: no log is running"; return USVMPC_E_ARG; }
    CAS_TRY(c, hipSetDevice(c->g->device));
    cascade_log_release(c);
    c->log.stop();
    return 0;
}

int usvmpc_cascade_log_info(usvmpc_cascade *c, int *records, long long *ticks, long long *missed, int *nsel)
{
    if (!c) return USVMPC_E_ARG;
    if (!c->log.on()) { c->err = "cascade_log_info: no log is running (usvmpc_cascade_log_start)"; return USVMPC_E_ARG; }
    if (records) *records = c->log.records();
    if (ticks) *ticks = c->log.ticks();
    if (missed) *missed = c->log.missed();
    if (nsel) *nsel = c->log.lay.nsel;
    return 0;
}

int usvmpc_cascade_log_read(usvmpc_cascade *c, const char *channel, int rec0, int nrec, int b0, int nb, void *out, size_t bytes)
{
    if (!c) return USVMPC_E_ARG;
    CasLogCopy cp;
    if (const char *why = c->log.read_desc(channel, rec0, nrec, b0, nb, &cp)) { c->err = why; return USVMPC_E_ARG; }
    if (!out || (long long)bytes != cp.bytes()) {
        c->err = "cascade_log_read: out must hold exactly " + std::to_string(cp.bytes()) + " bytes ([nrec][nb][" + std::to_string(cp.n) + "])";
        return USVMPC_E_ARG;
    }
    usvmpc_handle *h = c->g;
    const char *src = (const char *)c->log_buf[cp.channel];
    CAS_TRY(c, hipSetDevice(h->device));
    CAS_TRY(c, hipMemcpy2DAsync(out, (size_t)cp.width, src + cp.offset, (size_t)cp.pitch, (size_t)cp.width, (size_t)cp.rows, hipMemcpyDeviceToHost,
                                h->stream));
    CAS_TRY(c, hipStreamSynchronize(h->stream));
    return 0;
}

int usvmpc_cascade_log_device_ptr(usvmpc_cascade *c, const char *channel, void **dptr)
{
    if (!c || !dptr) return USVMPC_E_ARG;
    if (!c->log.on()) { c->err = "cascade_log_device_ptr: no log is running (usvmpc_cascade_log_start)"; return USVMPC_E_ARG; }
    const std::string s = channel ? channel : "";
    void *p = s == "state" ? c->log_buf[CAS_LOG_STATE] : s == "thrust" ? c->log_buf[CAS_LOG_THRUST] : s == "ref" ? c->log_buf[CAS_LOG_REF]
            : s == "err" ? c->log_buf[CAS_LOG_ERR] : s == "status" ? c->log_buf[CAS_LOG_STATUS] : nullptr;
    if (!p) { c->err = "cascade_log_device_ptr: '" + s + "' is no channel of the running log"; return USVMPC_E_ARG; }
    *dptr = p;
    return 0;
}

const char *usvmpc_cascade_last_error(usvmpc_cascade *c) { return c ? c->err.c_str() : g_cascade_create_err.c_str(); }

int usvmpc_set_stream(usvmpc_handle *h, void *stream)
{
    if (!h) return USVMPC_E_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    {
        const int rcf = mirror_flush(h);
        if (rcf) return rcf;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->hm.synced();
    {
        const int rcs = spec_cancel(h);
        if (rcs) return rcs;
        h->opt.pipeline = false; // (the caller's stream carries the caller's own ordering: nothing of this handle runs beside it)
        h->opt.handover_co = 0;
    }
    if (h->own_stream) (void)hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)stream;
    h->own_stream = false;
    return 0;
}

int usvmpc_sim_create(const usvmpc_sim_desc *d, usvmpc_sim **out)
{
    if (!d || !out) return USVMPC_E_ARG;
    *out = nullptr;
    int nx = 0, nu = 0;
    std::string err;
    const int rc = sim_check(*d, nx, nu, err);
    if (rc) {
        g_sim_create_err = "usvmpc_sim_create: " + err;
        return rc;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || d->device < 0 || d->device >= ndev) {
        g_sim_create_err = "usvmpc_sim_create: no usable HIP device (count " + std::to_string(ndev) + ", requested " + std::to_string(d->device) +
                           "); there is no CPU fallback";
        return USVMPC_E_NODEVICE;
    }
    usvmpc_sim *s = new usvmpc_sim();
    s->owner = &g_lib_tag;
    s->model = d->model; s->nx = nx; s->nu = nu; s->nz = nx + nu; s->B = d->batch; s->device = d->device;
    s->T = d->T; s->num_steps = d->num_steps; s->sens = d->sens_forw != 0;
    s->stream = nullptr; s->own_stream = true;
    s->x = s->u = s->xn = s->S = nullptr;
    auto fail = [&](hipError_t e, const char *what) {
        g_sim_create_err = std::string("usvmpc_sim_create: ") + what + ": " + hipGetErrorString(e);
        (void)hipFree(s->x); (void)hipFree(s->u); (void)hipFree(s->xn); (void)hipFree(s->S);
        if (s->stream) (void)hipStreamDestroy(s->stream);
        delete s;
        return USVMPC_E_HIP;
    };
    const size_t B = (size_t)s->B;
    hipError_t e;
    if ((e = hipSetDevice(s->device)) != hipSuccess) return fail(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking)) != hipSuccess) { s->stream = nullptr; return fail(e, "hipStreamCreate"); }
    if ((e = hipMalloc((void **)&s->x, B * nx * sizeof(double))) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMalloc((void **)&s->u, B * (nu ? nu : 1) * sizeof(double))) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMalloc((void **)&s->xn, B * nx * sizeof(double))) != hipSuccess) return fail(e, "hipMalloc");
    if (s->sens && (e = hipMalloc((void **)&s->S, B * nx * s->nz * sizeof(double))) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMemsetAsync(s->x, 0, B * nx * sizeof(double), s->stream)) != hipSuccess ||
        (e = hipMemsetAsync(s->u, 0, B * (nu ? nu : 1) * sizeof(double), s->stream)) != hipSuccess ||
        (e = hipMemsetAsync(s->xn, 0, B * nx * sizeof(double), s->stream)) != hipSuccess ||
        (s->S && (e = hipMemsetAsync(s->S, 0, B * nx * s->nz * sizeof(double), s->stream)) != hipSuccess) ||
        (e = hipStreamSynchronize(s->stream)) != hipSuccess)
        return fail(e, "hipMemsetAsync");
    *out = s;
    return 0;
}

int usvmpc_sim_destroy(usvmpc_sim *s)
{
    if (!s) return USVMPC_E_ARG;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    (void)hipFree(s->x); (void)hipFree(s->u); (void)hipFree(s->xn); (void)hipFree(s->S);
    if (s->own_stream) (void)hipStreamDestroy(s->stream);
    delete s;
    return 0;
}

int usvmpc_sim_set(usvmpc_sim *s, const char *field, const double *v, size_t n)
{
    if (!s) return USVMPC_E_ARG;
    if (!v) { s->err = "null buffer"; return USVMPC_E_ARG; }
    const std::string f(field ? field : "");
    if (f == "T") {
        if (n != 1) { s->err = "mismatching dimension for field 'T': expected 1, got " + std::to_string(n); return USVMPC_E_SIZE; }
        if (!(v[0] > 0.0) || !std::isfinite(v[0])) { s->err = "T must be positive and finite"; return USVMPC_E_ARG; }
        s->T = v[0];
        return 0;
    }
    int len = 0;
    double *dst = sim_field(s, f, true, len);
    if (!dst) { s->err = "unknown field '" + f + "' (set: \"x\", \"u\", \"T\")"; return USVMPC_E_FIELD; }
    if ((int)n != len) {
        s->err = "mismatching dimension for field '" + f + "': expected " + std::to_string(len) + ", got " + std::to_string(n);
        return USVMPC_E_SIZE;
    }
    if (len == 0) return 0;
    SIM_TRY(s, hipSetDevice(s->device));
    SIM_TRY(s, hipMemcpyAsync(dst, v, (size_t)s->B * len * sizeof(double), hipMemcpyHostToDevice, s->stream));
    SIM_TRY(s, hipStreamSynchronize(s->stream));
    return 0;
}

int usvmpc_sim_solve(usvmpc_sim *s)
{
    if (!s) return USVMPC_E_ARG;
    SIM_TRY(s, hipSetDevice(s->device));
    switch (s->model) {
#ifndef USV_GEN_ONLY
    case USVMPC_MODEL_USV: sim_launch_model<ModelM0>(s); break;
    case USVMPC_MODEL_GUIDANCE_CA1: sim_launch_model<ModelM1>(s); break;
    case USVMPC_MODEL_PF_CA: sim_launch_model<ModelM2>(s); break;
#endif
#ifdef USV_GEN_MODEL_HEADER
    case USVMPC_MODEL_GENERATED: sim_launch_model<ModelGen>(s); break;
#endif
    default: s->err = "no integrator kernel for this model in this library"; return USVMPC_E_ARG;
    }
    SIM_TRY(s, hipGetLastError());
    SIM_TRY(s, hipStreamSynchronize(s->stream));
    return 0;
}

int usvmpc_sim_get(usvmpc_sim *s, const char *field, double *out, size_t n)
{
    if (!s) return USVMPC_E_ARG;
    if (!out) { s->err = "null buffer"; return USVMPC_E_ARG; }
    const std::string f(field ? field : "");
    if (f == "T") {
        if (n != 1) { s->err = "mismatching dimension for field 'T': expected 1, got " + std::to_string(n); return USVMPC_E_SIZE; }
        out[0] = s->T;
        return 0;
    }
    if (f == "S_forw" && !s->sens) { s->err = "S_forw is not computed: the integrator was created with sens_forw = 0"; return USVMPC_E_FIELD; }
    int len = 0;
    const double *src = sim_field(s, f, false, len);
    if (!src) { s->err = "unknown field '" + f + "' (get: \"x\", \"S_forw\", \"T\")"; return USVMPC_E_FIELD; }
    if ((int)n != len) {
        s->err = "mismatching dimension for field '" + f + "': expected " + std::to_string(len) + ", got " + std::to_string(n);
        return USVMPC_E_SIZE;
    }
    SIM_TRY(s, hipSetDevice(s->device));
    SIM_TRY(s, hipMemcpyAsync(out, src, (size_t)s->B * len * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    SIM_TRY(s, hipStreamSynchronize(s->stream));
    return 0;
}

int usvmpc_sim_get_device_ptr(usvmpc_sim *s, const char *field, void **dptr)
{
    if (!s || !dptr) return USVMPC_E_ARG;
    const std::string f(field ? field : "");
    double *p = f == "x" ? s->x : f == "u" ? s->u : f == "x_next" ? s->xn : f == "S_forw" ? s->S : nullptr;
    if (!p) {
        s->err = f == "S_forw" ? "S_forw is not computed: the integrator was created with sens_forw = 0"
                               : "unknown field '" + f + "' (\"x\", \"u\", \"x_next\", \"S_forw\")";
        return USVMPC_E_FIELD;
    }
    *dptr = (void *)p;
    return 0;
}

int usvmpc_sim_set_stream(usvmpc_sim *s, void *stream)
{
    if (!s) return USVMPC_E_ARG;
    SIM_TRY(s, hipSetDevice(s->device));
    SIM_TRY(s, hipStreamSynchronize(s->stream));
    if (s->own_stream) (void)hipStreamDestroy(s->stream);
    s->stream = (hipStream_t)stream;
    s->own_stream = false;
    return 0;
}

const char *usvmpc_sim_last_error(usvmpc_sim *s) { return s ? s->err.c_str() : g_sim_create_err.c_str(); }

size_t usvmpc_device_bytes(usvmpc_handle *h) { return h ? h->bytes : 0; }

const char *usvmpc_last_error(usvmpc_handle *h) { return h ? h->err.c_str() : "null handle"; }

} // extern "C"
#endif // USV_MAIN

#ifndef USV_COND_SEPARATE // (one translation unit by default - generated-model and development builds; the shipped library compiles it on its own)
#include "cond_kernels.hip"
#endif
