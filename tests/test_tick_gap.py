"""tools/tick_gap.py: the per-tick budget between two QP launches, read from a kernel trace (CPU only)."""
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "tick_gap.py")
TRACE = os.path.join(ROOT, "profiles", "r06_g_kernel_trace.csv")


def _load():
    spec = importlib.util.spec_from_file_location("tick_gap", TOOL)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_round6_trace_medians():
    """The figures worked out by hand from the round-6 trace: 23 QP launches, median gap 4.14 ms over the ticks after the first two,
    median overrun of the speculative lineariser 3.67 ms."""
    tg = _load()
    recs = tg.ticks(tg.read_trace(TRACE))
    assert len(recs) == 23
    s = tg.summary(recs, skip=2)
    assert s["ticks"] == 20
    assert round(s["gap"]["median"], 2) == 4.14
    assert round(s["overrun"]["median"], 2) == 3.67
    assert 1.3 < s["gap"]["min"] < 1.4 and 5.3 < s["gap"]["max"] < 5.4
    assert 0.26 <= round(s["fixup"]["min"], 2) and round(s["fixup"]["max"], 2) <= 0.34
    assert abs(s["sort"]["median"] - 0.02) < 0.005 and abs(s["advance"]["median"] - 0.027) < 0.003
    # the first tick is linearised in full (nothing ran ahead for it), every later one by the speculative pass + fix-up
    assert recs[0]["full"] > 7.0 and recs[0]["overrun"] is None
    assert all(r["full"] == 0.0 and r["overrun"] is not None for r in recs[1:])
    # the overrun is the bulk of the gap
    for r in recs[2:-1]:
        assert r["overrun"] <= r["gap"] and r["overrun"] > 0.7 * r["gap"]


def test_synthetic_trace(tmp_path):
    """Two ticks with known times: a speculative launch that ends inside the gap, one that ends before the QP launch does."""
    lin = '"void usv_linearize<usv::ModelM2, 1, false, true, %d>(usv::DevPtrs, long)"'
    qp = '"void usv_qp_rti<usv::ModelM2, 1, false>(usv::DevPtrs, long, int, int, int)"'
    ms = 1000000
    rows = [
        (qp, 0, 60 * ms), (lin % 1, 1 * ms, 63 * ms), (lin % 2, 63 * ms, 64 * ms), ('"usv_sort_scan(int*, int*)"', 64 * ms, 64 * ms + 500000),
        (qp, 65 * ms, 120 * ms), (lin % 1, 66 * ms, 119 * ms), ('"usv_advance(usv::DevPtrs, int)"', 120 * ms, 121 * ms),
        (qp, 122 * ms, 180 * ms),
    ]
    p = tmp_path / "trace.csv"
    p.write_text("Kernel_Name,Start_Timestamp,End_Timestamp\n" + "".join("%s,%d,%d\n" % r for r in rows))
    tg = _load()
    recs = tg.ticks(tg.read_trace(str(p)))
    assert [r["gap"] for r in recs] == [5.0, 2.0, None]
    assert [r["overrun"] for r in recs] == [3.0, 0.0, None]
    assert recs[0]["fixup"] == 1.0 and recs[0]["sort"] == 0.5 and recs[1]["advance"] == 1.0 and recs[1]["fixup"] == 0.0
    s = tg.summary(recs, skip=0)
    assert s["ticks"] == 2 and s["gap"]["median"] == 3.5 and s["overrun"]["median"] == 1.5


def test_command_line():
    out = subprocess.run([sys.executable, TOOL, "--json", TRACE], check=True, capture_output=True, text=True).stdout
    s = json.loads(out)
    assert round(s["gap"]["median"], 2) == 4.14 and round(s["overrun"]["median"], 2) == 3.67
    txt = subprocess.run([sys.executable, TOOL, TRACE], check=True, capture_output=True, text=True).stdout
    assert "median over 20 ticks" in txt
