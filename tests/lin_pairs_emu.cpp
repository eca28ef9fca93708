// The paired lineariser (csrc/linearize.hpp run_pair*: two (instance, stage) pairs per 16-lane row) against the 16-lane form on the lane
// emulator (TEST-ONLY; tests/test_lin_pairs_emu.py compiles this file and links it to tests/emu/libusv_emu.so, which has the fibers).
// usv_emu_lin_pairs runs one order of both forms on the same inputs into two workspaces the caller compares plane by plane:
//   order 0  whole batch: MODE 0, run | run_pair
//   order 1  speculative, stage-major: MODE 1 with epoch[b] = ready[b] ? tick : tick - 1, run | run_pair (redo masks out)
//   order 2  fix-up, stage-major: MODE 2 over the caller's redo pattern
//   order 3  speculative in the retire order: MODE 3, run_item | run_pair_item
//   order 4  fix-up by groups: MODE 4, run_marked | run_pair_marked over the caller's redo pattern
// Returns the planes per stage (workspaces: [(N + 1)][Bp][npt][16] doubles), < 0: the model has no paired form / bad description.
#include "lanes.hpp"

#include "host_spec.hpp"
#include "linearize.hpp"
#include "models.hpp"

#include <cstring>
#include <vector>

using namespace usv;

namespace {

struct Job { const DevPtrs *P; long idx; };

template <class M, int KCH, bool SOFT, int MODE, bool PAIR>
void body(void *a)
{
    const Job *j = (const Job *)a;
    auto go = [&](auto multi) {
        using L = Linearize<M, KCH, SOFT, decltype(multi)::value, MODE>;
        if constexpr (MODE == 4) {
            if constexpr (PAIR) L::run_pair_marked(*j->P, j->idx, 0);
            else L::run_marked(*j->P, j->idx, 0);
        } else if constexpr (MODE == 3) {
            if constexpr (PAIR) L::run_pair_item(*j->P, j->idx);
            else L::run_item(*j->P, j->idx);
        } else {
            if constexpr (PAIR) L::run_pair(*j->P, j->idx);
            else L::run(*j->P, j->idx);
        }
    };
    if (j->P->spec->sim_steps > 1) go(std::true_type{});
    else go(std::false_type{});
}

template <class M, int KCH, bool SOFT, int MODE>
void both(DevPtrs P, const DevSpec &S, double *ws_ref, double *ws_pair, int *redo_ref, int *redo_pair)
{
    const long pairs = (long)(S.N + 1) * S.Bp;
    const long n_ref = MODE == 4 ? (long)S.Bp : pairs;
    const long n_pair = MODE == 4 ? (long)S.Bp : MODE == 3 ? lin_pair_retire_rows(S.N, S.Bp) : lin_pair_plain_rows(S.N, S.Bp);
    P.ws = ws_ref; P.redo = redo_ref;
    for (long i = 0; i < n_ref; i++) { Job j{&P, i}; lanes::run_group(i, &body<M, KCH, SOFT, MODE, false>, &j); }
    P.ws = ws_pair; P.redo = redo_pair;
    for (long i = 0; i < n_pair; i++) { Job j{&P, i}; lanes::run_group(i, &body<M, KCH, SOFT, MODE, true>, &j); }
}

template <class M, int KCH, bool SOFT>
int run(DevPtrs P, DevSpec &S, int order, const int *ready, double *ws_ref, double *ws_pair, int *redo_ref, int *redo_pair)
{
    if constexpr (!PairCols<M>::ENABLED) return -2;
    else {
        S.npt = WsLayout<M, KCH, SOFT, false>::NPT;
        const int tick = 7;
        std::vector<int> epoch(S.B);
        for (int b = 0; b < S.B; b++) epoch[b] = (ready == nullptr || ready[b]) ? tick : tick - 1;
        P.spec = &S; P.tick = tick; P.epoch = epoch.data(); P.redo_words = (S.N + 32) / 32;
        switch (order) {
        case 0: both<M, KCH, SOFT, 0>(P, S, ws_ref, ws_pair, redo_ref, redo_pair); break;
        case 1: both<M, KCH, SOFT, 1>(P, S, ws_ref, ws_pair, redo_ref, redo_pair); break;
        case 2: both<M, KCH, SOFT, 2>(P, S, ws_ref, ws_pair, redo_ref, redo_pair); break;
        case 3: both<M, KCH, SOFT, 3>(P, S, ws_ref, ws_pair, redo_ref, redo_pair); break;
        case 4: both<M, KCH, SOFT, 4>(P, S, ws_ref, ws_pair, redo_ref, redo_pair); break;
        default: return -3;
        }
        return S.npt;
    }
}

} // namespace

// perm_next: group -> instance of the planes written (inv_next its inverse); perm_cur: the "running" launch's map; any of them may be null (identity)
extern "C" int usv_emu_lin_pairs(const usvmpc_desc *d, int order, const double *x, const double *u, const double *yref, const double *yref_e,
                                 const int *ready, const int *perm_next, const int *inv_next, const int *perm_cur, double *ws_ref, double *ws_pair,
                                 int *redo_ref, int *redo_pair)
{
    DevSpec S;
    if (!build_spec(*d, S).empty()) return -1;
    DevPtrs P;
    std::memset(&P, 0, sizeof(P));
    P.x = const_cast<double *>(x); P.u = const_cast<double *>(u); P.yref = yref; P.yref_e = yref_e;
    P.perm = perm_next; P.inv_next = inv_next; P.perm_cur = perm_cur;
    if (d->model == USVMPC_MODEL_USV) return run<ModelM0, 0, false>(P, S, order, ready, ws_ref, ws_pair, redo_ref, redo_pair);
    if (d->model == USVMPC_MODEL_GUIDANCE_CA1) return run<ModelM1, 1, true>(P, S, order, ready, ws_ref, ws_pair, redo_ref, redo_pair);
    if (d->model == USVMPC_MODEL_PF_CA) return run<ModelM2, 1, false>(P, S, order, ready, ws_ref, ws_pair, redo_ref, redo_pair);
    return -3;
}

// entry (row j, variable c) of the packed stream of model id `model`: its position, -1 if it is not stored (the test looks the (ye, ak) entry up)
extern "C" int usv_emu_lin_pairs_entry(int model, int j, int c)
{
    auto pos = [&](auto m) {
        using MP = MatPack<decltype(m)>;
        int s = 0;
        for (int i = 0; i < j; i++) s += MP::count(i);
        return ((MP::row_mask(j) >> c) & 1u) ? s + MP::rank(MP::row_mask(j), c) : -1;
    };
    if (model == USVMPC_MODEL_USV) return pos(ModelM0{});
    if (model == USVMPC_MODEL_GUIDANCE_CA1) return pos(ModelM1{});
    if (model == USVMPC_MODEL_PF_CA) return pos(ModelM2{});
    return -1;
}

// first plane of the packed [B A] in a stage's window
extern "C" int usv_emu_lin_pairs_pmat(int model)
{
    if (model == USVMPC_MODEL_USV) return WsLayout<ModelM0, 0, false>::P_MAT;
    if (model == USVMPC_MODEL_GUIDANCE_CA1) return WsLayout<ModelM1, 1, true>::P_MAT;
    if (model == USVMPC_MODEL_PF_CA) return WsLayout<ModelM2, 1, false>::P_MAT;
    return -1;
}
