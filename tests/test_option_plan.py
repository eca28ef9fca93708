"""csrc/option_plan.hpp - the table of run-time options (names, checks, normalisation, where a value is stored, what it invalidates), the
Options struct with its defaults and parse_option - compiled with the host compiler (CPU only) and driven from a command line
(tests/option_plan_harness.cpp).

Every expected value is worked out by hand from usvmpc.hip's usvmpc_set_option and usvmpc_create as they stood before the table moved into
the header: a chain of `if (s == "...")` branches, each of which parsed, checked, stored and invalidated inline.

What the branches did with the caller's double v (N, nx, nu, K: the handle's sizes):
    v != 0                       obstacle_step_on_advance pipeline_linearize sort_two_ticks sort_by_difficulty aux_in_lds dynamic_rows handover_lds
                                 merge_box_rows cond_pred_corr static_obstacles (into DevSpec) keep_multipliers host_mirror (actions);
                                 pack_box_rows: (v != 0 && boxpack_ok)
    0 or 1, else "<name>: 0 or 1"   obstacle_tracks (1 with K = 0: "... no obstacle rows (K = 0)"), pf_predict, lin_pairs (1 on a model without pairs:
                                 "... does not declare the columns to integrate");  lin_force_modes: 0, 1 or 2
    v < 0 ? -1 : v > 0 ? 1 : 0   lds_workspace, wide;   handover_co: v < 0 ? -1 : v != 0 ? 1 : 0;   wide_waves: v < 0 ? -1 : v >= 4 ? 4 : 1
    pf_lh_margin                 !(v >= 0) or not finite: "pf_lh_margin must be finite and non-negative";  cpc_factor: !(v > 0): "cpc_factor must be positive"
    hpipm_mode                   v != (int) v or no profile of that number (0 .. 3): "hpipm_mode must be one of USVMPC_HPIPM_*"
    handover_iter                v > 1e6: "handover_iter out of range"; v < 0 ? -1 : (int) v
    handover_co_spin             !(1 <= v <= 2e9): "... out of range"; (int) v.   handover_co_wgs: !(0 <= v <= 1e6); (long) v
    instance_offset              !(0 <= v <= 2^53) or a fraction: "instance_offset must be a non-negative integer"
    qp_cond_N                    n2 = (int) v outside 0..N: "qp_cond_N must lie in 0..N"; 0 and N mean 0; n2 > 0: nx + ceil(N / n2) nu > 64: "... at most 64
                                 variables ...", then soft state bounds: "partial condensing (qp_cond_N) is not built for soft state bounds"
    max_waves (long) v, disturbance_mask (unsigned) v: plain casts - undefined for a NaN or a value the type does not hold, as were (int) v of
    qp_cond_N / hpipm_mode and of a NaN handover_iter.  Those inputs are now refused (USVMPC_E_ARG, the option's existing text, or
    "<name> out of range" where it had none); every value whose conversion was defined behaves as it did, negative max_waves included.
An unknown name: USVMPC_E_FIELD (-2), "unknown option '<name>'".

What they invalidated: spec_cancel came first for every option below obstacle_tracks, obstacle_step_on_advance, pf_predict and pf_lh_margin
(p, lh and the world are read by no lineariser); caps.reset(): max_waves aux_in_lds lds_workspace wide wide_waves dynamic_rows handover_lds
merge_box_rows pack_box_rows; cond_release: max_waves, and qp_cond_N when the value changed (with map_changed); layout_dirty: pack_box_rows;
tracks_dirty: static_obstacles (and obstacle_tracks when switched on: its hook); the DevSpec upload: cond_pred_corr cpc_factor hpipm_mode
static_obstacles pack_box_rows.  More than that (hooks): obstacle_tracks (who owns p), pf_predict (pf_apply_static), sort_by_difficulty (an
existing map is dropped), keep_multipliers (allocates), host_mirror (flush, free).

Defaults, from usvmpc_create: pipeline 1, sort 1, two-tick key 0, max_waves 0, lin_force 0, lin_pairs by model, aux_lds 1, lds / wide / wide_waves
-1, dynamic_rows 1, handover_iter -1, handover_lds 1, handover_co -1, spin limit 200000, co_wgs 0, mask ~0, offset 0, merge 1, step_on_advance 1,
pf_predict 1, pf_margin 0.2, cond_N2 0, tracks off."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "option_plan_harness.cpp")


def build(tmp_path_factory, name, *flags):
    exe = str(tmp_path_factory.mktemp(name) / "option_plan_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + CSRC, "-o", exe, SRC])
    return exe


# every case runs on the plain build and on one with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded)
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory, "option_plan")
    return build(tmp_path_factory, "option_plan_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run(exe, tokens):
    """One dict per printed line; `err` is the text to the end of the line, `fx` a set of effect names.  A sanitizer report ends the
    program with a message on stderr and a non-zero code."""
    r = subprocess.run([exe] + tokens, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        head, _, err = line.partition(" err=")
        w = head.split()
        d = {"kind": w[0], "err": err}
        d.update(kv.split("=", 1) for kv in w[1:] if "=" in kv)
        if w[0] == "name":
            d["name"] = w[1]
        if "fx" in d:
            d["fx"] = set() if d["fx"] == "-" else set(d["fx"].split("|"))
        out.append(d)
    return out


def check(exe, facts, name, cases):
    """cases: (value as the harness reads it, the normalised value - or the refusal's text)"""
    out = run(exe, facts.split() + ["set:%s:%s" % (name, v) for v, _ in cases])
    assert len(out) == len(cases)
    for (v, want), d in zip(cases, out):
        if isinstance(want, str):
            assert (d["rc"], d["err"]) == ("-1", want), (name, v, d)
        else:
            assert d["rc"] == "0" and d["err"] == "" and float(d["value"]) == want and not (float(d["value"]) == 0 and d["value"].startswith("-")), (name, v, d)
            # what the member then holds is the normalised value (the cast loses nothing)
            assert d["stored"] == "-" or float(d["stored"]) == want, (name, v, d)


FACTS = "N=6 nx=14 nu=2 K=3 pairs=1 bsoft=0 boxpack=1"   # usv_model_pf_ca
FLAGS = ["obstacle_step_on_advance", "pipeline_linearize", "sort_two_ticks", "sort_by_difficulty", "aux_in_lds", "dynamic_rows", "handover_lds",
         "merge_box_rows", "cond_pred_corr", "static_obstacles", "keep_multipliers", "host_mirror", "pack_box_rows"]
NAMES = sorted(FLAGS + ["obstacle_tracks", "pf_predict", "pf_lh_margin", "max_waves", "qp_cond_N", "lin_force_modes", "lin_pairs", "lds_workspace", "wide",
                        "wide_waves", "cpc_factor", "hpipm_mode", "handover_iter", "handover_co", "handover_co_spin", "handover_co_wgs",
                        "disturbance_mask", "instance_offset"])
INF = math.inf


def test_names(harness):
    assert len(NAMES) == 31
    assert sorted(d["name"] for d in run(harness, ["names"])) == NAMES


def test_unknown_and_null_names(harness):
    for d, shown in zip(run(harness, ["set:bogus:1", "set:Wide:1", "set:wide_:0", "set::1", "null:1", "set:bogus:nan"]), ["bogus", "Wide", "wide_", "", "", "bogus"]):
        assert (d["rc"], d["err"], d["fx"]) == ("-2", "unknown option '%s'" % shown, set()), d


def test_defaults(harness):
    want = dict(pipeline=1, sort_enabled=1, sort_two=0, max_waves=0, lin_force=0, lin_pairs=1, aux_lds=1, lds_mode=-1, wide_mode=-1, wide_waves=-1,
                dynamic_rows=1, handover_iter=-1, handover_lds=1, handover_co=-1, co_spin_limit=200000, co_wgs=0, noise_mask=4294967295,
                instance_offset=0, merge_rows=1, step_on_advance=1, pf_predict=1, pf_margin=0.2, cond_N2=0, tracks_on=0)
    for pairs in (1, 0):
        d, = run(harness, ["defaults:%d" % pairs])
        got = {k: float(v) for k, v in d.items() if k not in ("kind", "err")}
        assert got == dict(want, lin_pairs=pairs)


def test_flags(harness):
    for n in FLAGS:
        check(harness, FACTS, n, [("0", 0), ("1", 1), ("-0.0", 0), ("-2.5", 1), ("1e-300", 1), ("nan", 1), ("inf", 1), ("-inf", 1)])
    # "pack_box_rows" stays off where the rows do not fit
    check(harness, FACTS.replace("boxpack=1", "boxpack=0"), "pack_box_rows", [("0", 0), ("1", 0), ("nan", 0)])


def test_strict_choices(harness):
    for n in ("obstacle_tracks", "pf_predict", "lin_pairs"):
        bad = n + ": 0 or 1"
        check(harness, FACTS, n, [("0", 0), ("1", 1), ("-0.0", 0), ("2", bad), ("0.5", bad), ("-1", bad), ("1e-300", bad), ("nan", bad), ("inf", bad), ("-inf", bad)])
    bad = "lin_force_modes: 0, 1 or 2"
    check(harness, FACTS, "lin_force_modes", [("0", 0), ("1", 1), ("2", 2), ("3", bad), ("1.5", bad), ("-1", bad), ("nan", bad), ("inf", bad), ("-inf", bad)])
    # what the model and the sizes forbid: after the check of the value itself
    check(harness, FACTS.replace("pairs=1", "pairs=0"), "lin_pairs",
          [("0", 0), ("1", "lin_pairs: the model does not declare the columns to integrate"), ("2", "lin_pairs: 0 or 1")])
    check(harness, FACTS.replace("K=3", "K=0"), "obstacle_tracks",
          [("0", 0), ("1", "obstacle_tracks: this model has no obstacle rows (K = 0)"), ("2", "obstacle_tracks: 0 or 1")])


def test_tri_states(harness):
    for n in ("lds_workspace", "wide"):
        check(harness, FACTS, n, [("-1", -1), ("-0.001", -1), ("-inf", -1), ("0", 0), ("-0.0", 0), ("nan", 0), ("0.001", 1), ("1", 1), ("5", 1), ("inf", 1)])
    check(harness, FACTS, "handover_co", [("-1", -1), ("-0.5", -1), ("-inf", -1), ("0", 0), ("-0.0", 0), ("0.5", 1), ("1", 1), ("nan", 1), ("inf", 1)])
    check(harness, FACTS, "wide_waves", [("-1", -1), ("-0.5", -1), ("-inf", -1), ("0", 1), ("1", 1), ("3.9", 1), ("nan", 1), ("4", 4), ("100", 4), ("inf", 4)])


def test_reals(harness):
    bad = "pf_lh_margin must be finite and non-negative"
    check(harness, FACTS, "pf_lh_margin", [("0.2", 0.2), ("0", 0), ("-0.0", 0), ("1e300", 1e300), ("-1e-9", bad), ("nan", bad), ("inf", bad), ("-inf", bad)])
    bad = "cpc_factor must be positive"
    check(harness, FACTS, "cpc_factor", [("2", 2), ("1e-300", 1e-300), ("5e-324", 5e-324), ("inf", INF), ("0", bad), ("-0.0", bad), ("-1", bad), ("nan", bad), ("-inf", bad)])


def test_hpipm_mode(harness):
    bad = "hpipm_mode must be one of USVMPC_HPIPM_*"
    check(harness, FACTS, "hpipm_mode", [("0", 0), ("1", 1), ("2", 2), ("3", 3), ("-0.0", 0), ("4", bad), ("-1", bad), ("1.5", bad), ("nan", bad), ("inf", bad),
                                         ("-inf", bad), ("1e300", bad), ("-3e9", bad), ("4294967296", bad)])   # (the last: 0 after a wrap to 32 bits)


def test_hand_over(harness):
    bad = "handover_iter out of range"
    check(harness, FACTS, "handover_iter", [("-1", -1), ("-0.5", -1), ("-1e300", -1), ("-inf", -1), ("0", 0), ("-0.0", 0), ("20.7", 20), ("1e6", 1000000),
                                            ("1000000.5", bad), ("1000001", bad), ("inf", bad), ("nan", bad)])
    bad = "handover_co_spin out of range"
    check(harness, FACTS, "handover_co_spin", [("1", 1), ("200000.9", 200000), ("2e9", 2000000000), ("0.5", bad), ("0", bad), ("-1", bad), ("2000000001", bad),
                                               ("nan", bad), ("inf", bad), ("-inf", bad)])
    bad = "handover_co_wgs out of range"
    check(harness, FACTS, "handover_co_wgs", [("0", 0), ("-0.0", 0), ("256.5", 256), ("1e6", 1000000), ("-0.5", bad), ("1000001", bad), ("nan", bad), ("inf", bad), ("-inf", bad)])


def test_casts_that_were_undefined_are_refused(harness):
    bad = "max_waves out of range"   # long: [-2^63, 2^63); the doubles next to the ends are 2^63 - 1024 and -2^63 - 2048
    check(harness, FACTS, "max_waves", [("0", 0), ("64", 64), ("2.9", 2), ("-3.7", -3), ("-0.5", 0), ("-9223372036854775808", -2.0 ** 63),
                                        ("9223372036854774784", 2.0 ** 63 - 1024), ("9223372036854775808", bad), ("-9223372036854777856", bad),
                                        ("1e300", bad), ("nan", bad), ("inf", bad), ("-inf", bad)])
    bad = "disturbance_mask out of range"   # unsigned: (-1, 2^32)
    check(harness, FACTS, "disturbance_mask", [("0", 0), ("40", 40), ("-0.5", 0), ("-0.9999999999999999", 0), ("4294967295", 4294967295), ("4294967295.5", 4294967295),
                                               ("-1", bad), ("4294967296", bad), ("-1e300", bad), ("nan", bad), ("inf", bad), ("-inf", bad)])
    bad = "instance_offset must be a non-negative integer"
    check(harness, FACTS, "instance_offset", [("0", 0), ("-0.0", 0), ("4096", 4096), ("9007199254740992", 2.0 ** 53), ("9007199254740994", bad), ("-1", bad),
                                              ("0.5", bad), ("nan", bad), ("inf", bad), ("-inf", bad)])


def test_qp_cond_N(harness):
    bad = "qp_cond_N must lie in 0..N"
    check(harness, FACTS, "qp_cond_N", [("0", 0), ("-0.0", 0), ("-0.5", 0), ("6", 0), ("6.9", 0), ("3", 3), ("3.9", 3), ("1", 1), ("5", 5), ("7", bad), ("-1", bad),
                                        ("1e10", bad), ("-1e10", bad), ("1e300", bad), ("nan", bad), ("inf", bad), ("-inf", bad)])
    # one block's variables must fit a wave: nx + ceil(N / N2) nu <= 64.  N = 100, nx 14, nu 2: N2 = 4 -> 14 + 25 * 2 = 64; N2 = 3 -> 14 + 34 * 2 = 82
    wide = "qp_cond_N: a condensed stage may have at most 64 variables (nx + ceil(N / qp_cond_N) nu)"
    soft = "partial condensing (qp_cond_N) is not built for soft state bounds"
    big = FACTS.replace("N=6", "N=100")
    check(harness, big, "qp_cond_N", [("4", 4), ("3", wide), ("1", wide), ("100", 0), ("101", bad), ("50", 50)])
    # soft state bounds: refused unless the value means "off"; the size check comes first
    check(harness, big.replace("bsoft=0", "bsoft=1"), "qp_cond_N", [("0", 0), ("100", 0), ("4", soft), ("3", wide), ("101", bad)])


EFFECTS = {
    "keeps_ahead": {"obstacle_tracks", "obstacle_step_on_advance", "pf_predict", "pf_lh_margin"},
    "caps": {"max_waves", "aux_in_lds", "lds_workspace", "wide", "wide_waves", "dynamic_rows", "handover_lds", "merge_box_rows", "pack_box_rows"},
    "cond_release": {"max_waves", "qp_cond_N"},
    "map_changed": {"qp_cond_N"},
    "if_changed": {"qp_cond_N"},
    "layout_dirty": {"pack_box_rows"},
    "tracks_dirty": {"static_obstacles"},
    "upload_spec": {"cond_pred_corr", "cpc_factor", "hpipm_mode", "static_obstacles", "pack_box_rows"},
    "hook": {"obstacle_tracks", "pf_predict", "sort_by_difficulty", "keep_multipliers", "host_mirror"},
}


def test_effects_of_every_name(harness):
    out = run(harness, FACTS.split() + ["set:%s:0" % n for n in NAMES])
    for n, d in zip(NAMES, out):
        assert d["name"] == n and d["fx"] == {fx for fx, names in EFFECTS.items() if n in names}, d
    # a refusal still names its row's effects (the caller of parse_option performs none of them)
    d, = run(harness, ["set:max_waves:nan"])
    assert d["rc"] == "-1" and d["fx"] == {"caps", "cond_release"}


def test_no_value_reaches_an_undefined_conversion(harness):
    # (the sanitized build ends with a report on the first cast of a value its type does not hold; run asserts a clean exit)
    values = ["nan", "-nan", "inf", "-inf", "1e300", "-1e300", "1e19", "-1e19", "9223372036854775808", "-9223372036854777856", "4294967296", "-4294967297",
              "2147483648", "-2147483649", "2000000001", "0.5", "-0.5", "5e-324"]
    for facts in (FACTS, "N=100 nx=14 nu=2 K=0 pairs=0 bsoft=1 boxpack=0"):
        out = run(harness, facts.split() + ["set:%s:%s" % (n, v) for n in NAMES for v in values])
        assert len(out) == len(NAMES) * len(values) and all(d["rc"] in ("0", "-1") for d in out)
        for d in out:
            assert (d["rc"] == "-1") == (d["err"] != ""), d


def test_every_name_is_documented(harness):
    names = [d["name"] for d in run(harness, ["names"])]
    for doc in (os.path.join(ROOT, "include", "usvmpc.h"), os.path.join(ROOT, "INTEGRATION.md")):
        with open(doc) as f:
            text = f.read()
        assert [n for n in names if '"%s"' % n not in text] == [], doc
