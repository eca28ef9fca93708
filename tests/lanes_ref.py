"""What every numbered result of the lanes:: probe (mpc_collisionavoidance_amd/csrc/lanes_probe.hpp) is supposed to be: the plain reference
that tests/test_lanes_emu.py holds the CPU emulator (tests/emu/lanes.hpp) to and tests/test_gpu_lanes.py the device
(csrc/gfx950/lanes.hpp).  numpy and exact arithmetic only: index operations are index maps, a fused multiply-add is
float(Fraction(b) * Fraction(a) + Fraction(c)) - correctly rounded, so an unfused implementation differs in the last bit -, the
reductions are evaluated in the butterfly's fixed association (8, then 4, then 2, then 1; own operand first).  Nothing here is taken
from either header beyond the documented meaning of an operation.

Where IEEE 754 leaves the bits open - the sign of max / min of -0 and +0 - and for a signalling NaN, whose treatment the header did not
state, the reference does not guess: RULES below is what the MI355X returned, recorded in profiles/lanes_conformance.txt
("## recorded rules"), and both test files assert it.

Comparison is on bit patterns; a NaN compares as "is NaN", payload free."""
from fractions import Fraction

import numpy as np

# ---- numbering of lanes_probe.hpp (tests/test_lanes_emu.py checks the counts against the compiled probe)
S_A, S_B, S_C, S_D, S_E, S_FC, S_RED = range(7)
S_VA, S_VB, S_FA, S_FB, S_ST, NIN = range(S_RED + 6, S_RED + 12)
I_G = 0
I_BI, I_ANY, I_UNI, I_FIRST, I_XA, I_XW, NIIN = range(5, 12)
NRED = 6
_OUT = [("bcast", 16), ("ror", 15), ("gather", 5), ("fma_bc", 16), ("fma_bc.cancel", 1), ("fma_bc2", 1), ("fma_bc2.same_reg", 1), ("fma_bc3", 1),
        ("fma_bc3.acc_copy", 1), ("fma_bc4", 1), ("fma_bc4.b", 1), ("gsum", NRED), ("gmax", NRED), ("gmin", NRED), ("vmax", 1), ("vmax_abs", 1),
        ("vmax_abs2", 1), ("xrow_shfl", 3), ("xrow_max", 1), ("xrow_sum", 1), ("Xpose.row", 1), ("Xpose.wave", 1), ("Stash.get", 1), ("Stash.geth0", 1),
        ("Stash.geth1", 1), ("Stash16.get", 1), ("Planes.ld", 3), ("Planes.parked_ld", 2), ("PlanesLds", 1), ("st_shared", 1), ("ld_shared", 1),
        ("frcp", 1), ("frsqrt", 1), ("frcp2.a", 1), ("frcp2.b", 1)]
_IOUT = [("bcast_i", 16), ("lane_ids", 1), ("wave_any", 1), ("uniform", 1), ("wave_first_i", 1), ("count_one", 1), ("fetch_add.counter", 1),
         ("fetch_add", 1), ("claim.entry", 1), ("claim", 1), ("set_bits", 1), ("publish", 1), ("observe", 1)]


def _index(table):
    at, names, n = {}, [], 0
    for name, cnt in table:
        at[name] = n
        names += [name if cnt == 1 else "%s[%d]" % (name, i) for i in range(cnt)]
        n += cnt
    return at, names, n


O, OUT_NAMES, NOUT = _index(_OUT)
IO, IOUT_NAMES, NIOUT = _index(_IOUT)
NPL, PL_PAD = 3, 64
PARK_STORE, DEAD_STORE = 777.0, 555.0
CANARY = -6.02214076e23                    # fills the caller's allocation around the plane window
UNTOUCHED, IUNTOUCHED = 31337.25, -31337   # fill of out / iout: a result that is not produced keeps it
FAST = ("frcp", "frsqrt", "frcp2.a", "frcp2.b")   # measured in ulp on the device, not compared bit for bit

QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
NEG_QNAN = np.array([0xFFF8000000000123], dtype=np.uint64).view(np.float64)[0]
SNAN = np.array([0x7FF0000000000001], dtype=np.uint64).view(np.float64)[0]
SPECIALS = np.array([QNAN, NEG_QNAN, SNAN, 0.0, -0.0, np.inf, -np.inf, 1.5, -1.5, -3.0, 2.0])

# What the MI355X returned where IEEE 754 / the header leave it open (profiles/lanes_conformance.txt, "## recorded rules"):
#   max(+0, -0) and max(-0, +0)   through vmax, vmax_abs*, gmax, xrow_max (v_max_f64)  -> +0, whichever operand comes first
#   min(+0, -0) and min(-0, +0)   through gmin (fmin -> v_min_f64)                     -> -0, whichever operand comes first
#   a signalling NaN operand of max / min                                              -> NaN (a quiet NaN operand: the other operand)
RULES = {"max_zero_sign": +1, "min_zero_sign": -1, "snan_gives_nan": True}


def is_snan(x):
    b = np.asarray(x, dtype=np.float64).view(np.uint64)
    return np.isnan(x) & ((b & np.uint64(0x0008000000000000)) == 0)


def _maxmin(a, b, is_max):
    """max or min of two arrays as documented: the larger / smaller operand, the other operand for a NaN one; RULES for what that leaves open"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        r = np.where((a > b) if is_max else (a < b), a, b)
        r = np.where(np.isnan(b), a, r)
        r = np.where(np.isnan(a), b, r)
        zeros = (a == 0.0) & (b == 0.0) & (np.signbit(a) != np.signbit(b))
        r = np.where(zeros, np.copysign(0.0, RULES["max_zero_sign"] if is_max else RULES["min_zero_sign"]), r)
        if RULES["snan_gives_nan"]:
            r = np.where(is_snan(a) | is_snan(b), np.nan, r)
    return r


def max2(a, b):
    return _maxmin(a, b, True)


def min2(a, b):
    return _maxmin(a, b, False)


def ror(v, n):
    """rotate right by n lanes within the group: lane i receives the value of lane (i - n) mod 16"""
    return v[..., (np.arange(16) - n) & 15]


def butterfly(v, op):
    for n in (8, 4, 2, 1):
        v = op(v, ror(v, n))
    return v


def fma(b, a, c):
    """b * a + c with ONE rounding, elementwise"""
    b, a, c = np.broadcast_arrays(b, a, c)
    out = np.empty(b.shape)
    for i in np.ndindex(b.shape):
        out[i] = float(Fraction(float(b[i])) * Fraction(float(a[i])) + Fraction(float(c[i])))
    return out


def fma_chain(c, terms):
    """c += bcast<K>(b) * a for every (K, b, a) of terms, in that order"""
    for K, b, a in terms:
        c = fma(b[..., K:K + 1], a, c)
    return c


# ------------------------------------------------------------------ operands
def rows_launched(ngroups, block_threads):
    per = block_threads // 16
    return -(-ngroups // per) * per


def make_inputs(ngroups, block_threads, seed=0):
    """(in, iin, out0, iout0, planes0): operands distinct per (group, lane, slot) wherever a value's ORIGIN is what is checked"""
    rng = np.random.default_rng(1000 * seed + ngroups + block_threads)
    G = ngroups
    din = np.zeros((G, NIN, 16))
    for s in (S_A, S_B, S_C, S_D, S_E):
        din[:, s] = rng.uniform(1.0, 2.0, (G, 16)) * 2.0 ** rng.integers(-3, 4, (G, 16)) * rng.choice([-1.0, 1.0], (G, 16))
    din[:, S_FC] = -(din[:, S_B, 5:6] * din[:, S_A])            # minus the ROUNDED product: the fused result is its rounding error
    g, l = np.meshgrid(np.arange(G), np.arange(16), indexing="ij")
    red = din[:, S_RED:S_RED + NRED]
    # 0: cancellation (the association decides the bits)
    red[:, 0] = rng.uniform(1.0, 2.0, (G, 16)) * 10.0 ** rng.integers(-8, 17, (G, 16)) * rng.choice([-1.0, 1.0], (G, 16))
    big = rng.uniform(1e15, 1e16, (G, 4))
    for j in range(4):
        red[np.arange(G), 0, (np.arange(G) + 3 * j) % 16] = big[:, j]
        red[np.arange(G), 0, (np.arange(G) + 3 * j + 7) % 16] = -big[:, j]
    for s in (1, 2, 3):
        red[:, s] = rng.normal(0.0, 100.0, (G, 16))
    red[np.arange(G), 1, np.arange(G) % 16] = np.where(np.arange(G) % 2 == 0, np.inf, -np.inf)   # one infinity
    red[np.arange(G), 2, (5 * np.arange(G)) % 16] = np.inf                                       # both infinities
    red[np.arange(G), 2, (5 * np.arange(G) + 9) % 16] = -np.inf
    red[np.arange(G), 3, (3 * np.arange(G) + 1) % 16] = np.where(np.arange(G) % 3 == 0, NEG_QNAN, QNAN)  # a NaN in one lane
    red[:, 4] = np.where((g + l) % 2 == 0, QNAN, NEG_QNAN)                                         # ... in all lanes
    zbits = (np.arange(G) * 40503 + 0x9E37) & 0xFFFF                                               # signed zeros: all +0, all -0, then mixtures
    zbits[:2] = (0, 0xFFFF)[:min(G, 2)]
    red[:, 5] = np.where((zbits[:, None] >> np.arange(16)) & 1, -0.0, 0.0)
    pair = (g * 16 + l) % (len(SPECIALS) ** 2)                                                     # every ordered pair of the specials
    din[:, S_VA], din[:, S_VB] = SPECIALS[pair // len(SPECIALS)], SPECIALS[pair % len(SPECIALS)]
    la, lp = rng.uniform(-150, 150, (G, 16)), rng.uniform(-300, 300, (G, 16))
    din[:, S_FA], din[:, S_FB] = 10.0 ** la, 10.0 ** np.clip(lp - la, -300, 300)
    din[:, S_ST] = 16777217.0 + 2.0 * l + 32.0 * g            # odd integers above 2^24: none is a float
    assert din[:, S_ST].max() < 2.0 ** 25

    iin = np.zeros((G, NIIN, 16), dtype=np.int32)
    iin[:, I_G + 0] = l                                        # identity
    iin[:, I_G + 1] = 15 - l                                   # reversal
    iin[:, I_G + 2] = (g * 7 + 3) % 16                         # all lanes from one
    iin[:, I_G + 3] = 16 * (1 + (g + l) % 5) + (l * 5 + g) % 16   # sources above 15: only the low four bits count
    iin[:, I_G + 4] = -1 - ((l * 3 + g) % 40)                  # negative sources
    iin[:, I_BI] = rng.integers(-2 ** 31, 2 ** 31, (G, 16))
    iin[:, I_BI, 0] = -2 ** 31
    iin[:, I_BI, 1] = -1
    iin[:, I_BI, 2] = 2 ** 31 - 1
    iin[:, I_ANY] = ((g // 4) % 2 == 0) & (g % 4 == 2) & (l == 11)    # one lane of row 2 of every other wave
    iin[:, I_UNI] = 1000 + 17 * (g // 4)                       # the same in every lane of a wave
    iin[:, I_FIRST] = 5000 + 16 * g + l
    iin[:, I_XA] = (l * 11 + g * 5 + 16 * (l % 2)) % 32
    iin[:, I_XW] = (l * 13 + g * 29 + 7) % 64

    out0 = np.full((G, NOUT, 16), UNTOUCHED)
    iout0 = np.full((G, NIOUT, 16), IUNTOUCHED, dtype=np.int32)
    iout0[:, IO["count_one"], 0] = 100 * np.arange(G)
    iout0[:, IO["fetch_add.counter"], 0] = 0
    iout0[:, IO["claim.entry"], 0] = np.arange(G) + 3          # (read only at a wave's first group: gw + 3)
    iout0[:, IO["set_bits"], 0] = 1 << 30
    planes0 = np.full(2 * PL_PAD + G * NPL * 16 + 40, CANARY)
    planes0[PL_PAD:PL_PAD + G * NPL * 16] = rng.uniform(-1.0, 1.0, G * NPL * 16)
    return np.ascontiguousarray(din), np.ascontiguousarray(iin), out0, iout0, planes0


# ------------------------------------------------------------------ the reference
def reference(ngroups, block_threads, din, iin, out0, iout0, planes0):
    """(out, iout, planes) as the probe must leave them.  fetch_add tickets and claim winners are in canonical order (normalise())."""
    G, R = ngroups, rows_launched(ngroups, block_threads)
    eff = np.minimum(np.arange(R), G - 1)          # a row without a group computes on the last group's operands
    X, XI = din[eff], iin[eff]
    A, B, C, D, E = (X[:, s] for s in (S_A, S_B, S_C, S_D, S_E))
    lane = np.arange(16)
    row = np.arange(R)
    res = np.full((R, NOUT, 16), UNTOUCHED)
    ires = np.full((R, NIOUT, 16), IUNTOUCHED, dtype=np.int64)
    take = lambda v, src: np.take_along_axis(v, src & 15, axis=1)        # lane src (its low four bits) of the own group
    wave = lambda v: v.reshape(R // 4, 4, 16)                            # [wave][row of the wave][lane]
    xshfl = lambda v, mask: wave(v)[:, np.arange(4) ^ (mask >> 4)].reshape(R, 16)

    for k in range(16):
        res[:, O["bcast"] + k] = A[:, k:k + 1]
        ires[:, IO["bcast_i"] + k] = XI[:, I_BI, k:k + 1]
        res[:, O["fma_bc"] + k] = fma_chain(C, [(k, B, A)])
    for n in range(1, 16):
        res[:, O["ror"] + n - 1] = ror(A, n)
    for s in range(5):
        res[:, O["gather"] + s] = take(A, XI[:, I_G + s])
    ires[:, IO["lane_ids"]] = lane + 100 * (row[:, None] % 4) + 10000 * ((row[:, None] % 4) * 16 + lane) + 1000000 * (row[:, None] % (block_threads // 16))
    res[:, O["fma_bc.cancel"]] = fma_chain(X[:, S_FC], [(5, B, A)])
    res[:, O["fma_bc2"]] = fma_chain(C, [(3, B, A), (12, D, E)])
    res[:, O["fma_bc2.same_reg"]] = fma_chain(C, [(1, B, A), (2, B, A)])
    res[:, O["fma_bc3"]] = fma_chain(C, [(7, B, A), (0, D, E), (9, A, D)])
    res[:, O["fma_bc3.acc_copy"]] = fma_chain(C, [(2, B, A), (5, C, E), (1, D, C)])
    res[:, O["fma_bc4"]] = fma_chain(C, [(4, B, A), (11, D, E), (14, E, B), (6, A, D)])
    res[:, O["fma_bc4.b"]] = fma_chain(E, [(15, D, C), (8, A, B), (10, C, A), (13, B, E)])
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(NRED):
            v = X[:, S_RED + s]
            res[:, O["gsum"] + s] = butterfly(v, lambda a, b: a + b)
            res[:, O["gmax"] + s] = butterfly(v, max2)
            res[:, O["gmin"] + s] = butterfly(v, min2)
        va, vb = X[:, S_VA], X[:, S_VB]
        res[:, O["vmax"]] = max2(va, vb)
        res[:, O["vmax_abs"]] = max2(va, np.abs(vb))
        res[:, O["vmax_abs2"]] = max2(np.abs(va), np.abs(vb))
        for i, mask in enumerate((16, 32, 48)):
            res[:, O["xrow_shfl"] + i] = xshfl(A, mask)
        m = max2(B, xshfl(B, 16))
        res[:, O["xrow_max"]] = max2(m, xshfl(m, 32))
        s_ = B + xshfl(B, 16)
        res[:, O["xrow_sum"]] = s_ + xshfl(s_, 32)
    ires[:, IO["wave_any"]] = np.repeat((wave(XI[:, I_ANY]) != 0).any(axis=(1, 2)), 64).reshape(R, 16)
    first = lambda v: np.repeat(wave(v)[:, 0, 0], 64).reshape(R, 16)     # lane 0 of the wave
    ires[:, IO["uniform"]] = first(XI[:, I_UNI])
    assert (ires[:, IO["uniform"]] == XI[:, I_UNI]).all(), "the operand of uniform() must be wave-uniform"
    ires[:, IO["wave_first_i"]] = first(XI[:, I_FIRST])
    if block_threads == 64:
        both = np.concatenate([C, D], axis=1)                            # slots 0 .. 15: C, 16 .. 31: D, of the own row
        res[:, O["Xpose.row"]] = np.take_along_axis(both, XI[:, I_XA].astype(np.int64), axis=1)
        f32 = lambda v: v.astype(np.float32).astype(np.float64)
        res[:, O["Stash.get"]] = A
        res[:, O["Stash.geth0"]] = f32(X[:, S_ST])
        res[:, O["Stash.geth1"]] = f32(B)
    ew = wave(E).reshape(R // 4, 64)                                      # slot 16 r + l of the wave's area: lane l of its row r
    res[:, O["Xpose.wave"]] = np.take_along_axis(np.repeat(ew, 4, axis=0), XI[:, I_XW].astype(np.int64), axis=1)
    res[:, O["Stash16.get"]] = -3.0 - lane
    win = planes0[PL_PAD:PL_PAD + G * NPL * 16].reshape(G, NPL, 16)
    res[:G, O["Planes.ld"]:O["Planes.ld"] + 3] = win
    res[:, O["Planes.parked_ld"]:O["Planes.parked_ld"] + 2] = 0.0
    res[:, O["PlanesLds"]] = C[:, (lane + 1) & 15]
    res[:, O["st_shared"]] = D
    res[:, O["ld_shared"]] = D
    fa, fb = X[:, S_FA], X[:, S_FB]
    r_ = 1.0 / (fa * fb)                                                  # (the emulator's arithmetic: IEEE division; the device is measured)
    res[:, O["frcp"]], res[:, O["frsqrt"]], res[:, O["frcp2.a"]], res[:, O["frcp2.b"]] = 1.0 / fa, 1.0 / np.sqrt(fa), r_ * fb, r_ * fa

    out, iout, planes = out0.copy(), iout0.astype(np.int64), planes0.copy()
    out[:] = res[:G]
    keep = [IO[n] for n in ("count_one", "fetch_add.counter", "claim.entry", "set_bits")]
    mask = np.ones(NIOUT, dtype=bool)
    mask[keep] = False
    iout[:, mask] = ires[:G][:, mask]
    iout[:, IO["count_one"], 0] += 16
    iout[:, IO["publish"]] = 7 + np.arange(G)[:, None] + lane
    iout[:, IO["observe"]] = iout[:, IO["publish"]]
    for gw in range(0, G, 4):
        live = min(4, G - gw)
        iout[gw, IO["fetch_add.counter"], 0] += 16 * live
        iout[gw:gw + live, IO["fetch_add"]] = np.arange(16 * live).reshape(live, 16)
        iout[gw, IO["claim.entry"], 0] = -2 - (gw + 3)
        iout[gw:gw + live, IO["claim"]] = 0
        iout[gw, IO["claim"], 0] = 1
        iout[gw, IO["set_bits"], 0] |= 0xFFFF | (((1 << live) - 1) << 16)
    w = planes[PL_PAD:PL_PAD + G * NPL * 16].reshape(G, NPL, 16)         # (a view: the stores of the probe)
    w[:, 1], w[:, 2] = din[:, S_A], win[:, 0]
    return out, iout.astype(np.int32), planes


def normalise(iout, ngroups):
    """fetch_add tickets and the claim's winner do not depend on the order in which the lanes of a wave arrive: per wave, the tickets
    sorted, and the one winner (if it is exactly one) moved to the first lane"""
    iout = iout.copy()
    for gw in range(0, ngroups, 4):
        live = min(4, ngroups - gw)
        t = iout[gw:gw + live, IO["fetch_add"]]
        iout[gw:gw + live, IO["fetch_add"]] = np.sort(t.reshape(-1)).reshape(live, 16)
        c = iout[gw:gw + live, IO["claim"]]
        if sorted(c.reshape(-1).tolist()) == [0] * (16 * live - 1) + [1]:
            c[:] = 0
            c[0, 0] = 1
            iout[gw:gw + live, IO["claim"]] = c
    return iout


# ------------------------------------------------------------------ comparison
def same_bits(a, b):
    """elementwise: the same bit pattern, or both NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def disagreements(got, want, names, skip=()):
    """{result name: number of differing entries} over [group][result][16] arrays of doubles (bit patterns) or ints"""
    eq = same_bits(got, want) if got.dtype.kind == "f" else (got == want)
    bad = {}
    for r, name in enumerate(names):
        if name.split("[")[0] in skip:
            continue
        n = int((~eq[:, r]).sum())
        if n:
            bad[name] = n
    return bad


def tally(tallies, got, want, names, skip=()):
    """add, per primitive, the number of entries of `got` that equal `want` (and the number compared) to tallies[primitive] = [equal, compared]"""
    eq = same_bits(got, want) if got.dtype.kind == "f" else (got == want)
    for r, name in enumerate(names):
        p = name.split("[")[0]
        if p in skip:
            continue
        t = tallies.setdefault(p, [0, 0])
        t[0] += int(eq[:, r].sum())
        t[1] += int(eq[:, r].size)
