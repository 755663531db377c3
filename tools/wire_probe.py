"""What the wire program costs under closed-loop PI with a scan per step, at 10 000 x 8 read as 2 500 trains of 4
(every stage after the first linked), over 500 steps of 10 s, the chlorine loop on stage 0 only:
  (a) the loop on stage 0's own analyser (the reference point), one fused call;
  (b) (a) with a wire program whose every slot is -1, one fused call: its bits must equal (a)'s;
  (c) stage 0's chlorine_outlet slot wired to stage 3's analyser, one fused call;
  (d) the host loop (c) replaces -- one-step calls, sensor_readings(), the routing and the PI on the host
      (tests/wire_ref.py, tests/control_ref.py), write_holding: its bits must equal (c)'s.
The four alternate over five repeats, the order rotating; medians and ranges are reported.  Prints one JSON line.
   python tools/wire_probe.py [N] [n] [steps] [length]"""
import json, sys, time
import numpy as np
from probe_common import arguments, outputs, plant, rotate, same, timed_step, wt
from control_ref import ControlRef
from wire_ref import WireRef, WireScan, host_wired_loop

N, n, K, cols, bc = arguments(500)
L = int(sys.argv[4]) if len(sys.argv) > 4 else 4
DT = 10.0
stage = np.arange(N) % L
loop = wt.PILoop("chlorine_outlet", setpoint=np.asarray(cols["initial_chlorine"]) + 0.5, kp=0.5, ki=1e-3, bias=0.2, enable=stage == 0)
wire = wt.Wire("chlorine_outlet", 0, L - 1)


def run(name, rep=0):
    ens = plant(cols, bc, n)
    ens.set_trains(L)
    if name == "d":
        ctl = ControlRef(wt.control_block(N, loop, None), np.zeros(N))
        hs = WireScan(N, WireRef(wt.wire_block(N, L, wire), L), ctl=ctl, emulated=True, dt=DT)
        ens.synchronize()
        t0 = time.perf_counter()
        host_wired_loop(ens, hs, K, 1)
        ens.synchronize()
        dt = time.perf_counter() - t0
        out = outputs(ens, "boundary") + (ctl.st,)
    else:
        ens.enable_control(chlorine=loop)
        if name in "bc":
            ens.set_wires(*((wire,) if name == "c" else ()))
        _, dt = timed_step(ens, DT, K)
        out = outputs(ens, "boundary", "control_state")
    ens.close()
    return dt, out


run("c")                                         # module load, first launches
REPEATS = 5
times, med, last = rotate("abcd", REPEATS, run)
own_same, loop_same = same(last["a"][1], last["b"][1]), same(last["c"][1], last["d"][1])
moved = not same(last["a"][1], last["c"][1])
print(json.dumps({"N": N, "n": n, "steps": K, "length": L, "own_s": round(med["a"], 4), "all_own_program_s": round(med["b"], 4),
                  "wired_s": round(med["c"], 4), "host_loop_s": round(med["d"], 4),
                  "all_own_over_own": round(med["b"] / med["a"], 3), "wired_over_own": round(med["c"] / med["a"], 3),
                  "host_loop_over_wired": round(med["d"] / med["c"], 2), "repeats": REPEATS,
                  "all_s": {k: [round(t, 4) for t in v] for k, v in times.items()},
                  "range_s": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                  "all_own_bitwise_equal": bool(own_same), "wired_equals_host_loop_bitwise": bool(loop_same),
                  "wire_changes_the_run": bool(moved)}))
if not (own_same and loop_same and moved):
    sys.exit(1)
