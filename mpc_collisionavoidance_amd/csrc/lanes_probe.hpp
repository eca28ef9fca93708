// lanes_probe.hpp — every primitive of the lanes:: interface on caller-supplied operands, one numbered result each.
//
// ONE body, written only against lanes::, compiled twice: by hipcc against gfx950/lanes.hpp (kernel usv_debug_lanes, C entry
// usvmpc_debug_lanes) and by the host compiler against the emulator's tests/emu/lanes.hpp (usv_emu_lanes).  tests/lanes_ref.py states
// what each numbered result is supposed to be; tests/test_lanes_emu.py and tests/test_gpu_lanes.py hold the two implementations to it.
//
// Layouts (16 lanes innermost): in [group][NIN][16] doubles, iin [group][NIIN][16] ints, out [group][NOUT][16], iout [group][NIOUT][16].
// out and iout are in/out: a result the configuration does not produce, and every result of a row without a group, keeps what the
// caller put there; the atomics work on entries of iout the caller has initialised.
// WAVES = waves of the workgroup (1 or 4).  A workgroup takes the 4 * WAVES groups from `base` on, one per row.  Rows past the last
// group compute on a copy of the last group's operands and store nothing (control flow stays wave-uniform: no row leaves in front of
// a cross-lane operation); their Planes are parked at the end of the window, as QpIpm::solve parks a row that has run out of work.
// What is shared between rows or waves follows each primitive's contract: Xpose<., 4, false>, Xpose<., 1, true> and Stash<., 64> are
// wave-private areas of ONE-wave workgroups (WAVES == 1 only); Xpose<., 4, true> is per wave of a four-wave workgroup (WAVES == 4
// only); Stash<., 16> is one row's worth for all rows that share it, which all write the same value.
// No arithmetic of its own on the operands (a product followed by a sum would be contracted by one compiler and not by the other).
#pragma once
#include "lanes.hpp"
#include "sfor.hpp"

namespace usv {
namespace lanes_probe {

// operand slots
enum In { S_A = 0, S_B, S_C, S_D, S_E, S_FC, S_RED, S_VA = S_RED + 6, S_VB, S_FA, S_FB, S_ST, NIN };
enum IIn { I_G = 0, I_BI = I_G + 5, I_ANY, I_UNI, I_FIRST, I_XA, I_XW, NIIN };
// results
enum Out {
    O_BCAST = 0, O_ROR = O_BCAST + 16, O_GATHER = O_ROR + 15, O_FMA1 = O_GATHER + 5, O_FMA1C = O_FMA1 + 16, O_FMA2, O_FMA2S, O_FMA3, O_FMA3C, O_FMA4,
    O_FMA4B, O_GSUM, O_GMAX = O_GSUM + 6, O_GMIN = O_GMAX + 6, O_VMAX = O_GMIN + 6, O_VMAX_ABS, O_VMAX_ABS2, O_XSHFL, O_XMAX = O_XSHFL + 3, O_XSUM,
    O_XPOSE_ROW, O_XPOSE_WAVE, O_STASH, O_STASH_H0, O_STASH_H1, O_STASH16, O_PL, O_PARK = O_PL + 3, O_PLDS = O_PARK + 2, O_SHARED, O_SHARED_RD,
    O_FRCP, O_FRSQRT, O_FRCP2A, O_FRCP2B, NOUT
};
enum IOut { IO_BCASTI = 0, IO_IDS = IO_BCASTI + 16, IO_ANY, IO_UNIFORM, IO_FIRST, IO_COUNT, IO_FA_CTR, IO_FA, IO_CLAIM_ENTRY, IO_CLAIM, IO_BITS, IO_FLAG, IO_OBS, NIOUT };

constexpr int NPL = 3;       // planes per group of the Planes window
constexpr int PL_PAD = 64;   // doubles of the caller's allocation in front of the window (and at least as many behind it)
constexpr int NPL_LDS = 2;   // planes per row of the PlanesLds area (dynamic LDS: rows * NPL_LDS * 16 doubles)
constexpr double PARK_STORE = 777.0, DEAD_STORE = 555.0; // what the stores that must be dropped try to write

struct Args {
    const double *in;
    const int *iin;
    double *out;
    int *iout;
    double *planes;
    int ngroups;
};

template <int WAVES>
USV_DEV void run(const Args &a, long base)
{
    static_assert(WAVES == 1 || WAVES == 4, "waves of the workgroup");
    const int lane = lanes::lane();
    const long g = base + (long)lanes::block_row();
    const bool live = g < (long)a.ngroups;
    const long gc = live ? g : (long)a.ngroups - 1; // (a row without a group: the last group's operands)
    const long gw = g - (long)lanes::wave_row();     // first group of this wave: its entries of iout are the wave's atomics
    const double *in = a.in + gc * NIN * 16 + lane;
    const int *iin = a.iin + gc * NIIN * 16 + lane;
    double *out = a.out + gc * NOUT * 16 + lane;
    int *iout = a.iout + gc * NIOUT * 16 + lane;
    int *wout = a.iout + gw * NIOUT * 16;
    auto put = [&](int r, double v) { if (live) out[r * 16] = v; };
    auto puti = [&](int r, int v) { if (live) iout[r * 16] = v; };

    const double A = in[S_A * 16], B = in[S_B * 16], C = in[S_C * 16], D = in[S_D * 16], E = in[S_E * 16];

    // ---- broadcasts, rotations, gathers
    sfor<0, 16>([&](auto k) { put(O_BCAST + k, lanes::bcast<k>(A)); });
    const int bi = iin[I_BI * 16];
    sfor<0, 16>([&](auto k) { puti(IO_BCASTI + k, lanes::bcast_i<k>(bi)); });
    sfor<1, 16>([&](auto n) { put(O_ROR + n - 1, lanes::ror<n>(A)); });
    for (int s = 0; s < 5; s++) put(O_GATHER + s, lanes::gather(A, iin[(I_G + s) * 16]));
    puti(IO_IDS, lane + 100 * (int)lanes::wave_row() + 10000 * (int)lanes::wave_lane() + 1000000 * (int)lanes::block_row());

    // ---- the fused groups: remote b, own a, terms in the order given, one rounding each
    sfor<0, 16>([&](auto k) { double c = C; lanes::fma_bc<k>(c, B, A); put(O_FMA1 + k, c); });
    { double c = in[S_FC * 16]; lanes::fma_bc<5>(c, B, A); put(O_FMA1C, c); }   // (c = -round(B[5] * A): the result is the product's rounding error)
    { double c = C; lanes::fma_bc2<3, 12>(c, B, A, D, E); put(O_FMA2, c); }
    { double c = C; lanes::fma_bc2<1, 2>(c, B, A, B, A); put(O_FMA2S, c); }     // (one register as both remote sources)
    { double c = C; lanes::fma_bc3<7, 0, 9>(c, B, A, D, E, A, D); put(O_FMA3, c); }
    { double c = C; const double c0 = c; lanes::fma_bc3<2, 5, 1>(c, B, A, c0, E, D, c0); put(O_FMA3C, c); } // (sources that are the accumulator's old value)
    { double c = C; lanes::fma_bc4<4, 11, 14, 6>(c, B, A, D, E, E, B, A, D); put(O_FMA4, c); }
    { double c = E; lanes::fma_bc4<15, 8, 10, 13>(c, D, C, A, B, C, A, B, E); put(O_FMA4B, c); }

    // ---- reductions over the group
    for (int s = 0; s < 6; s++) {
        const double v = in[(S_RED + s) * 16];
        put(O_GSUM + s, lanes::gsum(v));
        put(O_GMAX + s, lanes::gmax(v));
        put(O_GMIN + s, lanes::gmin(v));
    }
    const double va = in[S_VA * 16], vb = in[S_VB * 16];
    put(O_VMAX, lanes::vmax(va, vb));
    put(O_VMAX_ABS, lanes::vmax_abs(va, vb));
    put(O_VMAX_ABS2, lanes::vmax_abs2(va, vb));

    // ---- across the rows of the wave
    put(O_XSHFL + 0, lanes::xrow_shfl(A, 16u));
    put(O_XSHFL + 1, lanes::xrow_shfl(A, 32u));
    put(O_XSHFL + 2, lanes::xrow_shfl(A, 48u));
    put(O_XMAX, lanes::xrow_max(B));
    put(O_XSUM, lanes::xrow_sum(B));
    puti(IO_ANY, lanes::wave_any(iin[I_ANY * 16] != 0) ? 1 : 0);
    puti(IO_UNIFORM, lanes::uniform(iin[I_UNI * 16]));
    puti(IO_FIRST, lanes::wave_first_i(iin[I_FIRST * 16]));

    // ---- the LDS exchange areas
    if constexpr (WAVES == 1) {
        using XR = lanes::Xpose<32, 4, false>;      // one area per row
        XR::put(lane, C);
        XR::put(16 + lane, D);
        XR::sync();
        put(O_XPOSE_ROW, XR::get(iin[I_XA * 16]));
        XR::sync();
    }
    {
        using XW = lanes::Xpose<64, (WAVES == 1 ? 1 : 4), true>; // one area per wave, shared by its four rows
        XW::put(16 * (int)lanes::wave_row() + lane, E);
        XW::sync();
        put(O_XPOSE_WAVE, XW::get(iin[I_XW * 16]));
        XW::sync();
    }
    if constexpr (WAVES == 1) {
        using ST = lanes::Stash<3, 64>;
        const double f = in[S_ST * 16];             // (not a float: both sides must round it alike)
        ST::put(0, A);
        ST::put(2, D);
        ST::puth(1, 0, f);
        ST::puth(1, 1, B);
        put(O_STASH, ST::get(0));
        put(O_STASH_H1, ST::geth(1, 1));
        ST::puth(1, 1, C);                          // (half 1 rewritten: half 0 must keep its value)
        put(O_STASH_H0, ST::geth(1, 0));
    }
    {
        using S16 = lanes::Stash<2, 16>;            // every row that shares it writes the same value
        S16::put(0, 0.5 + (double)lane);
        S16::put(1, -3.0 - (double)lane);
        lanes::lds_fence();
        put(O_STASH16, S16::get(1));
    }

    // ---- planes in HBM (a window inside the caller's allocation) and in LDS
    {
        const unsigned nbytes = (unsigned)a.ngroups * (unsigned)(NPL * 128);
        const double *win = a.planes + PL_PAD;
        const lanes::Planes W(win, nbytes, live ? lanes::Planes::lane_offset(g, NPL, lane) : nbytes);
        const double p0 = W.ld(0), p1 = W.ld(1), p2 = W.ld(2);
        put(O_PL + 0, p0); put(O_PL + 1, p1); put(O_PL + 2, p2);
        W.st(1, A);
        W.st(2, p0);
        const lanes::Planes P(win, nbytes, nbytes); // parked: loads 0, stores nothing
        put(O_PARK + 0, P.ld(0));
        put(O_PARK + 1, P.ld(2));
        P.st(0, PARK_STORE);
        P.st(2, PARK_STORE);
    }
    {
        const unsigned off = lanes::block_row() * (unsigned)(NPL_LDS * 16) + (unsigned)lane;
        const unsigned nb = lanes::block_row() * (unsigned)(NPL_LDS * 16) + (unsigned)((lane + 1) & 15);
        const lanes::PlanesLds L(off, true), Dead(off, false), Next(nb, true);
        L.st(0, B);
        L.st(1, C);
        Dead.st(1, DEAD_STORE);
        lanes::lds_fence();
        put(O_PLDS, Next.ld(1));                    // the neighbouring lane's entry
    }

    // ---- atomics and hand-over accesses, within this launch
    if (live) {
        lanes::count_one(a.iout + (g * NIOUT + IO_COUNT) * 16);
        iout[IO_FA * 16] = lanes::fetch_add(wout + IO_FA_CTR * 16);
        iout[IO_CLAIM * 16] = lanes::claim(wout + IO_CLAIM_ENTRY * 16, (int)gw + 3) ? 1 : 0;
        lanes::set_bits(wout + IO_BITS * 16, (1 << lane) | (1 << (16 + (int)lanes::wave_row())));
        lanes::st_shared(out + O_SHARED * 16, D);
        lanes::publish(iout + IO_FLAG * 16, 7 + (int)g + lane);
        lanes::drain_stores();
        out[O_SHARED_RD * 16] = lanes::ld_shared(out + O_SHARED * 16);
        iout[IO_OBS * 16] = lanes::observe(iout + IO_FLAG * 16);
    }

    // ---- reciprocals (measured, not compared bit for bit)
    const double fa = in[S_FA * 16], fb = in[S_FB * 16];
    double ia, ib;
    lanes::frcp2(fa, fb, ia, ib);
    put(O_FRCP, lanes::frcp(fa));
    put(O_FRSQRT, lanes::frsqrt(fa));
    put(O_FRCP2A, ia);
    put(O_FRCP2B, ib);
}

} // namespace lanes_probe
} // namespace usv
