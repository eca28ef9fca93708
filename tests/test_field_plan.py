"""csrc/field_plan.hpp - the table of caller-visible fields, the arena's layout and the host mirror's bookkeeping - compiled with the host
compiler (CPU only) and driven from a command line (tests/field_plan_harness.cpp).  Three layers: the table, the copies the bookkeeping
emits for a sequence of calls, and a model check of the whole against the direct path.

Every expected value is worked out by hand from usvmpc.hip as it stood before the table and the bookkeeping moved into the header.

The table.  lookup(field, stage, set) gave (array, per-stage length, stages, caller stage of slot 0):
    x (nx, N+1, 0)  u (nu, N, 0)  x0 (nx, 1, 0)  yref (ny, N, 0) - at stage == N: yref_e's array (ny_e, 1, N)  yref_e (ny_e, 1, 0)
    p (2K, N+1, 0)  lh (K, N, 0);  get only: pi (nx, N, 1)  sl, su (K, N, 0)  res, nlp_res (4, 1, 0)  obs_tmin (1, 1, 0)
    lam, t (nlam, N+1, 0) once lam_out / t_out exist;  anything else, a set of a get-only name included: "unknown field", USVMPC_E_FIELD (-2)
copy_field first normalised the stage of res / nlp_res / obs_tmin / x0 / yref_e to (stage < 0 ? -1 : 0), ran the export for a get of lam / t,
handed obs_pos / obs_vel (set, get) and clearance / clearance_min (get) to tracks_field, set pf_stale on a set of yref / yref_e and told the
lineariser's schedule of a set of x / u / yref / yref_e.  Stage check (after the lookup, the size check and the return for an empty field): a
whole-field call (stage < 0) passes; a one-stage array takes only its own stage ("stage out of range", code 2 below); else stage - offset must lie
in [0, stages) ("stage S out of range for field", code 1).  field_index: x u x0 yref yref_e p lh -> arena slots 0 1 3 4 5 6 7 (yref at stage N: 5);
status is slot 2.  usvmpc_get_int knew status qp_iter qp_status sqp_iter; usvmpc_get_device_ptr obs_pos obs_vel and the seventeen names
x u x0 yref yref_e p lh pi sl su status qp_iter qp_status res obs_tmin nlp_res sqp_iter.
Sizes: ny = nx + nu, ny_e = nx (host_spec.hpp); M0 usv_model nx 5 nu 2 K 0; M1 usv_model_guidance_ca1 nx 8 nu 1; M2 usv_model_pf_ca nx 14 nu 2.

The arena.  usvmpc_create laid [x | u | status | x0 | yref | yref_e | p | lh] out with lengths B (N+1) nx 8, B N nu 8, B 4, B nx 8, B N ny 8, B ny_e 8,
B (N+1) 2K 8, B N K 8 bytes, each piece starting at the next multiple of 256.  The bookkeeping cases use N 10, nx 3, nu 2, ny 5, ny_e 3, K 2:
    B = 1: lengths 264 160 4 24 400 24 352 160 -> offsets 0 512 768 1024 1280 1792 2048 2560, end 2816
    B = 3: lengths 792 480 12 72 1200 72 1056 480 -> offsets 0 1024 1536 1792 2048 3328 3584 4864, end 5376
    B = 1, K = 0: p and lh are empty -> offsets .. 1792 2048 2048, end 2048

The bookkeeping (copy_field's mirror path, mirror_flush).  A set of an arena field on a handle with a mirror: wait if a copy is in flight, write
the mirror, then - one stage with B > 1: under a handed-out device pointer one 2-D copy (offset field + stage * row, pitch stages * row, width row, B
rows) at once, else the stage is marked; whole field or B == 1: the field's ONE dirty range [lo, hi) widens to cover [0, len) or the stage's row.  A get
is answered by the mirror only for x / u, after a solve has brought them back and while no device pointer is out.  mirror_flush: per field one 2-D copy per
run of consecutive marked stages (offset field + a * row, width (b - a + 1) * row, B rows), then per dirty range one copy, extended over the following
fields while this one is dirty to its end and the next one from 0.  After a solve one copy brings bytes [0, offset of x0) back.

The model check states its two conditions where it generates the scripts (field_plan_harness.cpp, Sim::model), both from properties the header names:
(b) with B == 1 the external writer behind a handed-out pointer acts only directly after a flush point - and with B > 1 it likewise never writes a
field whose whole-field set is still deferred: a deferred range would land on top of it (strided stage sets went up at once and carry no condition);
(a) with B == 1, per-stage sets of a field whose device rows the mirror has not seen name one stage between two flushes - the range over two
stages would upload the mirror's stale rows in between."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "field_plan_harness.cpp")


def build(tmp_path_factory, name, *flags):
    exe = str(tmp_path_factory.mktemp(name) / "field_plan_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + CSRC, "-o", exe, SRC])
    return exe


# every case runs on the plain build and on one with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded)
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory, "field_plan")
    return build(tmp_path_factory, "field_plan_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run(exe, tokens):
    """One dict per printed line (`kind`: row, q, layout, op, model), integers where they are integers; an op carries its `copies`:
    (kind, offset, pitch, width, rows) in the order they were emitted."""
    r = subprocess.run([exe] + tokens.split(), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        d = {"kind": w[0]}
        for kv in w[1:]:
            if "=" in kv:
                k, v = kv.split("=", 1)
                d[k] = int(v) if v.lstrip("-").isdigit() else v
        if w[0] == "copy":
            out[-1]["copies"].append((w[1], d["off"], d["pitch"], d["width"], d["rows"]))
            continue
        if w[0] == "op":
            d["copies"] = []
        out.append(d)
    return out


def ops(exe, sizes, script):
    out = [d for d in run(exe, sizes + " " + script) if d["kind"] == "op"]
    assert len(out) == len(script.split())
    return out


def copies(exe, sizes, script):
    return [c for d in ops(exe, sizes, script) for c in d["copies"]]


# ---- 1. the table
SET = {"x", "u", "x0", "yref", "yref_e", "p", "lh", "obs_pos", "obs_vel"}
GET = SET | {"pi", "sl", "su", "res", "obs_tmin", "nlp_res", "lam", "t", "clearance", "clearance_min"}
GET_INT = {"status", "qp_iter", "qp_status", "sqp_iter"}
DEV = {"x", "u", "x0", "yref", "yref_e", "p", "lh", "pi", "sl", "su", "status", "qp_iter", "qp_status", "res", "obs_tmin", "nlp_res", "sqp_iter",
       "obs_pos", "obs_vel"}
NAMES = sorted(GET | GET_INT)
SLOT = {"x": 0, "u": 1, "status": 2, "x0": 3, "yref": 4, "yref_e": 5, "p": 6, "lh": 7}
MODELS = {"M0": (5, 2, 0), "M1": (8, 1, 3), "M2": (14, 2, 4)}  # nx, nu, K


def sizes(nx, nu, K, N=6, B=2):
    return "B=%d N=%d nx=%d nu=%d ny=%d ny_e=%d K=%d nlam=7" % (B, N, nx, nu, nx + nu, nx, K)


def test_rights_and_flags_of_every_name(harness):
    assert len(NAMES) == 23
    rows = {d["name"]: d for d in run(harness, " ".join("row:" + n for n in NAMES + ["bogus", "X", "yref_", ""])) if d["kind"] == "row"}
    for n in ("bogus", "X", "yref_"):
        assert rows[n]["found"] == 0
    for n in NAMES:
        r = rows[n]
        assert r["found"] == 1
        assert (r["set"], r["get"], r["get_int"], r["dev"]) == (int(n in SET), int(n in GET), int(n in GET_INT), int(n in DEV)), n
        assert r["slot"] == SLOT.get(n, -1) and r["int"] == int(n in GET_INT), n
        # the four flags of copy_field, and the track fields
        assert r["whole"] == int(n in ("res", "nlp_res", "obs_tmin", "x0", "yref_e")), n
        assert r["lin"] == int(n in ("x", "u", "yref", "yref_e")), n
        assert r["pf"] == int(n in ("yref", "yref_e")), n
        assert r["export"] == int(n in ("lam", "t")), n
        assert r["track"] == int(n in ("obs_pos", "obs_vel", "clearance", "clearance_min")), n


def test_set_and_get_accept_what_lookup_accepted(harness):
    # through resolve: the names lookup knew (the track fields never reached it: they are tracks_field's, which has its own messages, and
    # resolve accepts them by their rights); lam / t are unknown until exported; a null name (the harness cannot pass one) is find_field's nullptr
    sz = sizes(*MODELS["M1"])
    for n in NAMES + ["bogus"]:
        s, g = [d["rc"] for d in run(harness, sz + " q:set:%s:0 q:get:%s:0" % (n, n))]
        assert s == (0 if n in SET else -2), n
        assert g == (0 if n in GET - {"lam", "t"} else -2), n
    for n in ("lam", "t"):
        a, b, c = run(harness, sz + " q:get:%s:2 exported=1 q:get:%s:2 q:set:%s:2" % (n, n, n))
        assert a["rc"] == -2 and c["rc"] == -2
        assert (b["rc"], b["n"], b["stages"], b["stage_off"], b["slot"]) == (0, 7, 7, 0, -1)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_length_stages_and_stage_offset(harness, model):
    nx, nu, K = MODELS[model]
    N = 6
    want = {"x": (nx, N + 1, 0), "u": (nu, N, 0), "x0": (nx, 1, 0), "yref": (nx + nu, N, 0), "yref_e": (nx, 1, 0), "p": (2 * K, N + 1, 0),
            "lh": (K, N, 0), "pi": (nx, N, 1), "sl": (K, N, 0), "su": (K, N, 0), "res": (4, 1, 0), "nlp_res": (4, 1, 0), "obs_tmin": (1, 1, 0)}
    for n, w in want.items():
        q, = run(harness, sizes(nx, nu, K, N) + " q:get:%s:1" % n)
        assert (q["rc"], q["as"], q["n"], q["stages"], q["stage_off"]) == (0, n) + w, n
        assert q["check"] == 0 and q["slot"] == SLOT.get(n, -1)


def test_yref_at_stage_N_is_yref_e(harness):
    sz = sizes(*MODELS["M2"], N=6, B=3)
    a, b, c, d = run(harness, sz + " q:set:yref:5 q:set:yref:6 q:set:yref:7 q:set:yref:-1")
    assert (a["as"], a["slot"], a["n"], a["stages"], a["stage_off"], a["check"]) == ("yref", 4, 16, 6, 0, 0)
    # stage N: yref_e's array, addressed as that array's only stage - one piece of B * ny_e * 8 bytes; both flags as for either name
    assert (b["as"], b["slot"], b["n"], b["stages"], b["stage_off"], b["check"]) == ("yref_e", 5, 14, 1, 6, 0)
    assert (b["off"], b["width"], b["rows"], b["lin"], b["pf"]) == (0, 3 * 14 * 8, 1, 1, 1)
    assert (c["as"], c["check"]) == ("yref", 1)        # past N: yref's own range check
    assert (d["as"], d["check"], d["width"], d["rows"]) == ("yref", 0, 3 * 6 * 16 * 8, 1)
    # one stage of yref: B rows of ny doubles, a horizon apart
    assert (a["off"], a["pitch"], a["width"], a["rows"]) == (5 * 16 * 8, 6 * 16 * 8, 16 * 8, 3)


def test_whole_only_fields_ignore_the_stage(harness):
    sz = sizes(*MODELS["M1"])
    for n in ("res", "nlp_res", "obs_tmin", "x0", "yref_e"):
        for stage, norm in ((-1, -1), (-7, -1), (0, 0), (3, 0), (99, 0)):
            q, = run(harness, sz + " q:get:%s:%d" % (n, stage))
            assert (q["rc"], q["stage"], q["check"], q["rows"]) == (0, norm, 0, 1), (n, stage)
    # not so a one-stage array reached under another name, nor any staged field
    q, = run(harness, sz + " q:get:x:99")
    assert (q["stage"], q["check"]) == (99, 1)


def test_pi_is_get_only_and_starts_at_stage_1(harness):
    sz = sizes(*MODELS["M2"], N=6)
    s, g0, g1, g6, g7, gw = run(harness, sz + " q:set:pi:1 q:get:pi:0 q:get:pi:1 q:get:pi:6 q:get:pi:7 q:get:pi:-1")
    assert s["rc"] == -2
    assert [g["check"] for g in (g0, g1, g6, g7, gw)] == [1, 0, 0, 1, 0]
    assert (g1["off"], g6["off"], g1["pitch"], g1["width"]) == (0, 5 * 14 * 8, 6 * 14 * 8, 14 * 8)


def test_stage_ranges(harness):
    sz = sizes(*MODELS["M2"], N=6)
    for q, want in zip(run(harness, sz + " q:set:x:6 q:set:x:7 q:set:u:5 q:set:u:6 q:set:p:6 q:set:lh:6 q:set:x:-1 q:set:lh:-3"), [0, 1, 0, 1, 0, 1, 0, 0]):
        assert q["check"] == want, q


def test_arena_layout(harness):
    def lay(tokens):
        out = run(harness, tokens + " layout")
        return [d["off"] for d in out], [d["len"] for d in out][:-1], out[-1]
    off, ln, end = lay("B=1 N=10 nx=3 nu=2 ny=5 ny_e=3 K=2")
    assert ln == [264, 160, 4, 24, 400, 24, 352, 160] and off == [0, 512, 768, 1024, 1280, 1792, 2048, 2560, 2816]
    off, ln, end = lay("B=3 N=10 nx=3 nu=2 ny=5 ny_e=3 K=2")
    assert ln == [792, 480, 12, 72, 1200, 72, 1056, 480] and off == [0, 1024, 1536, 1792, 2048, 3328, 3584, 4864, 5376]
    off, ln, end = lay("B=1 N=10 nx=3 nu=2 ny=5 ny_e=3 K=0")
    assert ln[6:] == [0, 0] and off[5:] == [1792, 2048, 2048, 2048]
    assert end["max"] == 1 << 20 and end["mirrored"] == 1
    # the mirror's limit, 1 MiB, is inclusive.  B = 1, nx = 1, nu = ny = ny_e = K = 0: x is 8 (N + 1) bytes, status and x0 one 256-byte piece each, the
    # rest empty: N = 131007 -> 1048064 + 512 = 1048576 exactly; N = 131008 -> x pads to 1048320: 1048832
    assert lay("B=1 N=131007 nx=1 nu=0 ny=0 ny_e=0 K=0")[2]["mirrored"] == 1
    assert lay("B=1 N=131008 nx=1 nu=0 ny=0 ny_e=0 K=0")[2]["mirrored"] == 0


# ---- 2. the bookkeeping
S1 = "B=1 N=10 nx=3 nu=2 ny=5 ny_e=3 K=2"
S3 = "B=3 N=10 nx=3 nu=2 ny=5 ny_e=3 K=2"
PROTOCOL = " ".join("set:yref:%d set:p:%d set:lh:%d" % (k, k, k) for k in range(10)) + " set:p:10 set:yref:10 set:x0:0"


def test_reference_protocol_is_one_copy(harness):
    # 3 N + 3 setters: no copy, no wait; yref, yref_e, p, lh and x0 are then dirty from 0 to their ends - x0 (offset 1024) first in the arena,
    # each dirty to its end and the next from 0: ONE copy up to the end of lh, 2560 + 160 = 2720
    out = ops(harness, S1, PROTOCOL + " flush")
    for d in out[:-1]:
        assert (d["rc"], d["served"], d["wait"], d["copies"]) == (0, 1, 0, [])
    assert out[-1]["copies"] == [("up", 1024, 1696, 1696, 1)]


def test_reference_protocol_without_obstacles_stops_at_yref_e(harness):
    # K = 0: the sets of p / lh are sets of nothing (returned before any mirror work); the chain ends with yref_e: 1792 + 24 = 1816
    out = ops(harness, S1.replace("K=2", "K=0"), PROTOCOL + " flush")
    assert all(d.get("empty") == 1 for d, t in zip(out, PROTOCOL.split()) if t.startswith(("set:p", "set:lh")))
    assert out[-1]["copies"] == [("up", 1024, 792, 792, 1)]


def test_property_a_one_range_per_field_on_a_single_instance(harness):
    # B = 1, stages 2 and 9 of lh (rows of 16 bytes): the range [32, 160) - one copy that spans stages 2 .. 9, in between included
    assert copies(harness, S1, "set:lh:2 set:lh:9 flush") == [("up", 2560 + 32, 128, 128, 1)]
    # (order does not matter, nor does a stage set twice)
    assert copies(harness, S1, "set:lh:9 set:lh:2 set:lh:9 flush") == [("up", 2560 + 32, 128, 128, 1)]


def test_strided_stages_go_up_as_runs(harness):
    # B = 3, stages 2, 3, 5 of lh (pitch 160, row 16): two 2-D copies of three rows - the run 2 .. 3 and stage 5 - and no range
    assert copies(harness, S3, "set:lh:2 set:lh:5 set:lh:3 flush") == [("up", 4864 + 32, 160, 32, 3), ("up", 4864 + 80, 160, 16, 3)]
    # runs are per field: stage 9 of yref (pitch 400, row 40) and stage 0 of yref do not join, fields in arena order
    assert copies(harness, S3, "set:lh:0 set:yref:9 set:yref:0 flush") == [("up", 2048, 400, 40, 3), ("up", 2048 + 360, 400, 40, 3), ("up", 4864, 160, 16, 3)]


def test_whole_field_and_stage_of_the_same_field_both_go_up(harness):
    want = [("up", 4864 + 64, 160, 16, 3), ("up", 4864, 480, 480, 1)]
    assert copies(harness, S3, "set:lh:-1 set:lh:4 flush") == want
    assert copies(harness, S3, "set:lh:4 set:lh:-1 flush") == want
    # a one-stage field of several instances is a whole-field set: x0 (72 bytes) as a range, merged with nothing (yref is clean)
    assert copies(harness, S3, "set:x0:0 flush") == [("up", 1792, 72, 72, 1)]


def test_strided_stage_goes_up_at_once_under_a_device_pointer(harness):
    out = ops(harness, S3, "devptr set:lh:2 flush")
    assert out[1]["copies"] == [("now", 4864 + 32, 160, 16, 3)] and out[2]["copies"] == []
    # ... and that copy is in flight: the next set waits, once
    out = ops(harness, S3, "devptr set:lh:2 set:lh:3 set:lh:4")
    assert [d["wait"] for d in out[1:]] == [0, 1, 1]
    # handing the pointer out uploads what was pending
    out = ops(harness, S3, "set:lh:2 devptr flush")
    assert out[1]["copies"] == [("up", 4864 + 32, 160, 16, 3)] and out[2]["copies"] == []


def test_property_b_single_instance_stays_deferred_under_a_device_pointer(harness):
    out = ops(harness, S1, "devptr set:lh:2 flush")
    assert out[1]["copies"] == [] and out[2]["copies"] == [("up", 2560 + 32, 16, 16, 1)]
    # ... and so does a whole-field set of several instances
    out = ops(harness, S3, "devptr set:lh:-1 flush")
    assert out[1]["copies"] == [] and out[2]["copies"] == [("up", 4864, 480, 480, 1)]


@pytest.mark.parametrize("sz,x0_off", [(S1, 1024), (S3, 1792)])
def test_gets_served_from_the_mirror(harness, sz, x0_off):
    out = ops(harness, sz, "get:x:1 get:u:-1 solve get:x:1 get:u:0 get:x:-1 get:x0:0 get:yref:2 get:lh:-1 devptr get:x:1 get:u:0 solve sync get:x:1")
    assert [d["served"] for d in out[:2]] == [0, 0]                # nothing has come back yet
    assert out[2]["copies"] == [("back", 0, x0_off, x0_off, 1)]   # [x | u | status] in one copy
    assert [(d["served"], d["wait"]) for d in out[3:6]] == [(1, 1), (1, 0), (1, 0)]   # (the first get waits for the read-back)
    assert [d["served"] for d in out[6:9]] == [0, 0, 0]            # x0 and the inputs: never
    assert [d["served"] for d in out[10:12]] == [0, 0]             # a device pointer is out
    assert out[14]["served"] == 0                                  # ... for good
    # usvmpc_solve's status comes from the same read-back, pointer or not; not before a solve, not without a mirror
    assert [d["served"] for d in ops(harness, sz, "status solve status devptr solve status drop status") if "served" in d] == [0, 1, 1, 0]
    assert [d["served"] for d in ops(harness, sz + " mirror=0", "solve status get:x:1 set:x:1") if "served" in d] == [0, 0, 0]


def test_set_waits_for_a_copy_in_flight(harness):
    out = ops(harness, S1, "set:yref:0 solve set:yref:0 set:yref:1 flush set:lh:0 flush sync set:lh:1 solve sync set:x:2")
    assert [d["wait"] for d in (out[0], out[2], out[3], out[5], out[8], out[11])] == [0, 1, 0, 1, 0, 0]


def test_second_flush_is_empty(harness):
    out = ops(harness, S3, PROTOCOL + " set:x:-1 set:u:3 flush flush solve")
    # x whole (792 bytes at 0), u stage 3 (pitch 160, row 16) and the protocol's stages: 2-D copies first (u, yref as one run of 10 stages, p
    # stages 0 .. 10 as one run, lh), then the ranges x and [x0 | (yref clean) ] and yref_e: x0 and yref_e are not adjacent dirty ranges
    assert out[-3]["copies"] == [("up", 1024 + 48, 160, 16, 3), ("up", 2048, 400, 400, 3), ("up", 3584, 352, 352, 3), ("up", 4864, 160, 160, 3),
                                 ("up", 0, 792, 792, 1), ("up", 1792, 72, 72, 1), ("up", 3328, 72, 72, 1)]
    assert out[-2]["copies"] == [] and out[-1]["copies"] == [("back", 0, 1792, 1792, 1)]


def test_dropping_the_mirror_flushes_first(harness):
    out = ops(harness, S1, "set:lh:1 set:x0:0 drop set:lh:2 get:lh:2 flush solve get:x:0")
    assert out[2]["copies"] == [("up", 1024, 24, 24, 1), ("up", 2560 + 16, 16, 16, 1)]
    assert [d["served"] for d in (out[3], out[4], out[7])] == [0, 0, 0]
    assert out[5]["copies"] == [] and out[6]["copies"] == []      # nothing is staged, nothing comes back


# ---- 3. the model check: the emitted copies carried out on byte buffers, against the direct path
def test_scripted_interleavings_behave_like_the_direct_path(harness):
    # tests/test_gpu_api.py::test_host_mirror_staging_is_invisible, restated (the harness exits non-zero where a get or a flush point differs)
    script = ("get:x:-1 " + PROTOCOL + " solve sync status get:x:1 get:u:0 get:x:-1 get:u:-1 set:x:5 get:x:-1 get:x:5 get:x:6 advance get:x0:0 "
              "set:lh:2 solve sync status get:x:-1 get:u:-1 get:lh:-1 set:x0:0 advance get:x0:0 devptr ext:u:-1 get:u:-1 solve set:yref:0 sync "
              "get:x:-1 status solve sync get:x:-1 get:u:-1")
    for sz in (S1, S3, S1.replace("K=2", "K=0"), S3 + " mirror=0"):
        assert len(ops(harness, sz, script)) == len(script.split())
    # the front end between the caller's sets; an external writer between strided sets (B = 3: any time)
    ops(harness, S3, "set:yref:-1 frontend set:yref:3 set:p:2 solve get:yref:-1 get:p:-1 devptr set:yref:0 ext:yref:0 set:yref:1 ext:yref:1 ext:yref:5 solve get:yref:-1")
    ops(harness, S1, "set:yref:-1 frontend set:yref:3 set:p:2 solve get:yref:-1 get:p:-1 devptr flush ext:yref:0 set:yref:0 solve get:yref:-1")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [2, 0])
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_random_interleavings_behave_like_the_direct_path(harness, B, K, seed):
    # N = 4, nx 3, nu 2, ny 4, ny_e 2 (the harness's defaults); 3000 operations; odd seeds hand a device pointer out half way, every third
    # gives the mirror up at three quarters
    out, = run(harness, "B=%d K=%d model:%d:3000" % (B, K, seed))
    assert out["kind"] == "model" and out["ops"] == 3000
    assert out["gets"] > 300 and out["served"] > 30 and out["flushes"] > 300 and out["waits"] > 30 and out["copies"] > 300
