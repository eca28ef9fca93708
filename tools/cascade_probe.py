#!/usr/bin/env python3
"""What the cascade's coupling costs on the device (guidance.Cascade; kernels usv_cascade_refs, usv_cascade_step), low level N = 100:
  - usv_cascade_refs on a rewriting tick (a guidance tick: every instance's 100 reference rows) and on an idle one, and usv_cascade_step, from
    events on the cascade's stream, with the bytes each moves / its time beside it;
  - a whole low-level tick and a whole guidance tick, and the low-level solve's own time in its generated library (kernel_ms);
  - the coupling done by the HOST instead: synchronise, read x_1, heading and speed back, numpy (scenario.cascade_ll_outputs /
    cascade_plant_step / cascade_ll_inputs), upload x0, yref and yref_e.

--log: the same with the cascade's log (every channel, every tick: kernel usv_cascade_record ahead of usv_cascade_step) and the tracked cost
of both layers (one more usv_cost_track launch per solve) switched on, the launches they add timed on their own, and the alternative they
replace: the host synchronises at every tick and reads state, thrusts, set-points, errors and both layers' status back.

    python tools/cascade_probe.py --batch 8192 65536 --write          -> profiles/cascade_probe.txt
    python tools/cascade_probe.py --batch 8192 65536 --log --write    -> profiles/cascade_log_probe.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/cascade_probe.py --batch 8192 --trace-only [--log]    (a run of its own)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpc_collisionavoidance_amd import BatchOcpSolver, scenario, usv_models  # noqa: E402
from mpc_collisionavoidance_amd.guidance import Cascade, GuidanceFrontEnd  # noqa: E402

N, K, DT, LN, RATIO = 100, 8, 0.05, 100, 5


def stack(B):
    m = scenario.make_ca_missions(B, 6, seed=0)
    g = BatchOcpSolver(usv_models.make_ocp("usv_model_guidance_ca1", N * DT, N, K), B)
    fe = GuidanceFrontEnd(g)
    ll = BatchOcpSolver(usv_models.make_ocp("usv_model_low_level", LN * DT / RATIO, LN), B)
    fe.reset(m["waypoints"], m["pose"][:, 2])
    fe.set_world(m["world"])
    cas = Cascade(fe, ll, ratio=RATIO)
    cas.reset(m["pose"], np.column_stack([m["vel"], np.zeros(B)]))
    return g, fe, ll, cas


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def log_on(cas, ticks):
    """every channel at every tick, and the realised cost of both layers"""
    cas.start_log(ticks, err=True)
    cas.track_cost()


def host_log(g, fe, ll, cas):
    """what a logged tick keeps on the device, read back by the host instead (ms)"""
    t0 = time.perf_counter()
    ll.sync()
    st = cas.state()
    pub = fe.publish()
    _, _, eu, epsi = scenario.cascade_ll_outputs(ll.get("x", 1), pub["heading"], pub["speed"], st["state"])
    word = [s.get_int(f) for s in (ll, g) for f in ("status", "qp_iter")]
    rec = (st["state"], st["thrust"], pub["heading"], pub["speed"], eu, epsi, word)
    return 1e3 * (time.perf_counter() - t0), rec


def probe(B, periods, lines, log=False):
    g, fe, ll, cas = stack(B)
    st = cas._stream
    if log:
        log_on(cas, RATIO * (periods + 1))
    for _ in range(RATIO):                                        # warm-up: one guidance period
        cas.tick()
    g.sync()
    refs_w, refs_i, step, tick_ll, tick_g, solve, trk_g, trk_l = [], [], [], [], [], [], [], []
    for p in range(periods):
        for i in range(RATIO):
            gt = cas.guidance_tick()
            if gt and log:                                       # (Cascade.guidance, the tracking launch timed on its own)
                t0 = timed(st, lambda: (fe.prepare(), g.solve_async()))
                trk_g.append(timed(st, g.track_cost_now))
                t0 += trk_g[-1] + timed(st, lambda: fe.publish(fetch=False))
            else:
                t0 = timed(st, cas.guidance) if gt else 0.0
            (refs_w if gt else refs_i).append(timed(st, cas.refs))
            solve.append(timed(st, ll.solve_async))
            if log:
                trk_l.append(timed(st, ll.track_cost_now))
            step.append(timed(st, cas.step))                     # (with a log: usv_cascade_record and usv_cascade_step)
            (tick_g if gt else tick_ll).append(t0 + (refs_w if gt else refs_i)[-1] + solve[-1] + step[-1] + (trk_l[-1] if log else 0.0))
    writes = cas.state()["yref_writes"]
    lin, qp = ll.kernel_ms(min(len(solve), 32))
    # ---- the same coupling through the host
    host = []
    pub = fe.publish()
    s, past = cas.state()["state"], cas.state()["past_thrust"]
    for i in range(3):
        t0 = time.perf_counter()
        ll.sync()
        x1 = ll.get("x", 1)
        pub = fe.publish()
        thr, past, _, _ = scenario.cascade_ll_outputs(x1, pub["heading"], pub["speed"], s)
        s = scenario.cascade_plant_step(s, thr, DT / RATIO)
        x0, row = scenario.cascade_ll_inputs(s, past, pub["heading"], pub["speed"])
        ll.set("x0", 0, x0)
        ll.set_all("yref", np.tile(row[:, None, :], (1, LN, 1)))
        ll.set("yref", LN, row[:, :8])
        ll.sync()
        host.append(1e3 * (time.perf_counter() - t0))
    med = lambda v: float(np.median(v)) if len(v) else float("nan")
    if log:
        info = cas.log_info()
        host_rec = [host_log(g, fe, ll, cas)[0] for _ in range(3)]
        rbytes = B * (6 + 2 + 2) * 8 + B * 2 * 4 + B * 4         # a record: 92 bytes per instance
    wbytes = B * (LN * 10 + 8 + 8) * 8 + B * (6 + 2 + 2 + 2) * 8      # yref + yref_e + x0 written; vessel, past, set-points, last read
    ibytes = B * 8 * 8 + B * (6 + 2 + 2 + 2) * 8
    sbytes = B * (8 + 6 + 2 + 4) * 8 + B * (6 + 2 + 2 + 4) * 8 + B * 4
    lines += ["B = %d, low level N = %d, guidance N = %d / K = %d, ratio %d, %d guidance periods" % (B, LN, N, K, RATIO, periods),
              "  usv_cascade_refs, rewriting tick   %8.3f ms   %7.1f MB  %7.1f GB/s   (yref_writes %d)" % (med(refs_w), wbytes / 1e6, wbytes / med(refs_w) / 1e6, writes),
              "  usv_cascade_refs, idle tick        %8.3f ms   %7.1f MB  %7.1f GB/s" % (med(refs_i), ibytes / 1e6, ibytes / med(refs_i) / 1e6),
              "  usv_cascade_step                   %8.3f ms   %7.1f MB  %7.1f GB/s" % (med(step), sbytes / 1e6, sbytes / med(step) / 1e6),
              "  low-level solve (enqueue to done)  %8.3f ms   (kernel_ms: lineariser %.3f + QP %.3f)" % (med(solve), float(np.median(lin)), float(np.median(qp))),
              "  low-level tick                     %8.3f ms   guidance tick %8.3f ms" % (med(tick_ll), med(tick_g)),
              "  coupling net of the QP launches    %8.3f ms (rewriting)  %8.3f ms (idle);  done by the host instead: %8.1f ms" % (
                  med(refs_w) + med(step), med(refs_i) + med(step), med(host))]
    if log:
        lines += ["  with the log (every channel, every tick: %d records, %d missed) and the tracked cost of both layers on:" % (info["records"], info["missed"]),
                  "  usv_cascade_record + usv_cascade_step  %6.3f ms (the step line above)   a record: %.1f MB, %d B per instance" % (med(step), rbytes / 1e6, rbytes // B),
                  "  usv_cost_track, low level          %8.3f ms   guidance %8.3f ms (guidance ticks only)" % (med(trk_l), med(trk_g)),
                  "  coupling net of the QP launches, log and tracking included  %8.3f ms (rewriting)  %8.3f ms (idle)" % (
                      med(refs_w) + med(step) + med(trk_l) + med(trk_g), med(refs_i) + med(step) + med(trk_l)),
                  "  the same quantities read back by the host at a tick (synchronise, state, publish, x_1, status x 4): %8.1f ms" % med(host_rec)]
    cas.close(); ll.close(); g.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--periods", type=int, default=4)
    ap.add_argument("--trace-only", action="store_true", help="run the ticks and print nothing (under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--log", action="store_true", help="the cascade's log and the tracked cost of both layers switched on")
    ap.add_argument("--write", nargs="?", const="", default=None, metavar="FILE",
                    help="also write the lines to FILE (default profiles/cascade_probe.txt, with --log profiles/cascade_log_probe.txt)")
    a = ap.parse_args()
    if a.write == "":
        a.write = os.path.join(ROOT, "profiles", "cascade_log_probe.txt" if a.log else "cascade_probe.txt")
    lines = ["# tools/cascade_probe.py --batch %s --periods %d%s" % (" ".join(map(str, a.batch)), a.periods, " --log" if a.log else "")]
    for B in a.batch:
        if a.trace_only:
            g, fe, ll, cas = stack(B)
            if a.log:
                log_on(cas, RATIO * a.periods)
            for _ in range(RATIO * a.periods):
                cas.tick()
            g.sync()
            cas.close(); ll.close(); g.close()
        else:
            probe(B, a.periods, lines, a.log)
            print("\n".join(lines[-(12 if a.log else 7):]), flush=True)
    if a.write and not a.trace_only:
        with open(a.write, "w") as f:
            f.write("\n".join(lines) + "\n")
