"""What a link program with a scan per outer step costs, three ways, at 10 000 x 8 over 120 steps of 10 s:
  (a) the host loop it needs without the feature: write_holding() of what the restated command slots leave of the PI's
      words, step(dt, 1, fused=False), sensor_readings(), input_image(), the link and the PI programs in numpy
      (tests/link_ref.py, control_ref.py), every step;
  (b) one fused call with both programs on the device, a scan per step;
  (c) the same call without the link program, as the reference point.
Every reactor has three slots: the outlet analyser of the chlorine loop delayed by 0 to 7 scans (one reactor per delay:
the curve of harm against network delay), the pH probe's polls lost with probability 0.3 and a timeout of 50 s into an
open circuit, and the chlorine command replayed from a tape of 8 scans over the second half of the run.  Checks that
(a) and (b) give bitwise the same states, readings, boundaries, PI and link state and rings, and prints one JSON line.
The two fused calls run five times each in rotating order and report their medians, every run is listed, and the host
loop runs once.  Times are reported, nothing is asserted about them.
   python tools/link_probe.py [N] [n] [steps]"""
import json, sys, time
import numpy as np
from probe_common import arguments, outputs, pi_loops, plant, rotate, same, timed_step, wt
from control_ref import ControlRef
from link_ref import LS_N_LOST, LS_N_TIMEOUT, LinkRef, LinkThenInject
from program_helpers import HostScan

N, n, K, cols, bc = arguments(120)
DT = 10.0
SEED = 20261021
chlorine, acid, u = pi_loops(cols, N)
slots = (wt.Link.delay("chlorine_outlet", np.arange(N) % 8),
         wt.Link.loss("pH_outlet", 0.3, timeout=5 * DT, fail=1),
         wt.Link.replay("chlorine_flow_rate", 8, start=(K // 2) * DT))
blocks = dict(control=wt.control_block(N, chlorine, acid), link=wt.link_block(N, *slots))

OUT = ("sensor_readings", "boundary")

warm = plant(cols, bc, n)                                   # module load, first launches
warm.set_links(*slots, seed=SEED); warm.step(DT, n_steps=2, download=False); warm.link_state(); warm.close()


def host_loop():
    ens = plant(cols, bc, n)
    ctl, lnk = ControlRef(blocks["control"], np.zeros(N)), LinkRef(blocks["link"], seed=SEED)
    ens.synchronize()
    t0 = time.perf_counter()
    HostScan(N, ctl=ctl, inj=LinkThenInject(lnk), emulated=True, dt=DT).run(ens, K, 1, fused=False, image=True)
    dt = time.perf_counter() - t0
    out = outputs(ens, *OUT)
    ens.close()
    return dt, out, (ctl.st, lnk.st) + lnk.in_order()


def fused(link):
    ens = plant(cols, bc, n)
    ens.enable_control(chlorine, acid)
    if link:
        ens.set_links(*slots, seed=SEED)
    _, dt = timed_step(ens, DT, K)
    out = outputs(ens, *OUT)
    st = (ens.control_state().block(), ens.link_state().block()) + tuple(ens.link_ring()) if link else None
    ens.close()
    return dt, out, st


ta, out_a, st_a = host_loop()
times, median, last = rotate(("link", "none"), 5, lambda v, rep: fused(v == "link"))
tb, tc = median["link"], median["none"]
(_, out_b, st_b), _ = last["link"], last["none"]
equal = same(out_a, out_b) and same(st_a, st_b)
ls = st_b[1]
print(json.dumps({"N": N, "n": n, "steps": K, "host_loop_s": round(ta, 4), "fused_link_s": round(tb, 4),
                  "without_link_s": round(tc, 4), "loop_over_fused": round(ta / tb, 2), "link_over_without": round(tb / tc, 3),
                  "fused_runs_s": {v: [round(t, 4) for t in ts] for v, ts in times.items()},
                  "polls_lost": int(ls[1, LS_N_LOST].sum()), "scans_timed_out": int(ls[1, LS_N_TIMEOUT].sum()),
                  "bitwise_equal": bool(equal)}))
if not equal:
    sys.exit(1)
