"""What model predictive dosing control with a scan per outer step costs, four ways, at 10 000 x 8 over 120 steps of 10 s:
  (a) the host loop it needs without the feature: step(dt, 1, fused=False), sensor_readings(), input_image(), the
      controllers in numpy (tests/mpc_ref.py), write_holding(), every step;
  (b) one fused call with both controllers on the device (ReactorEnsemble.set_mpc), a scan per step;
  (c) the same call with plant I/O but no controller, as the reference point;
  (d) the call of (b) with every loop disabled: the section is entered and does nothing.
The chlorine loop runs on the outlet analyser with a horizon of 64 and a period of one scan, the acid loop on the inlet
pH probe with a horizon of 24 and a period of two (the pH probes are in their 1800 s warm-up for the whole of the default
run: that loop waits, held at every scan, and the JSON line's execution counts say so).  Checks that (a)
and (b) give bitwise the same states, readings, images, boundaries, controller states and predictions, and (c) and (d)
the same plant, and prints one JSON line.  The three fused calls run five times each in rotating order and report their
medians, and every run is listed: on one MI355X some first step calls after set_mpc took about 27 ms longer than the
others, with the loops enabled or disabled, which a single run per variant would report as the variant's cost; the host
loop runs once.  Times are reported, nothing is asserted about them.
   python tools/mpc_probe.py [N] [n] [steps]"""
import json, sys, time
import numpy as np
from probe_common import arguments, outputs, plant, rotate, same, timed_step, wt
from mpc_ref import LoopOwners, MpcRef
from program_helpers import HostScan

N, n, K, cols, bc = arguments(120)
DT = 10.0
u = np.random.default_rng(3).random((2, N))
chlorine = wt.DMCLoop.from_fopdt("chlorine_outlet", cols["initial_chlorine"] + 0.5, 2.0, 60.0, 30.0, DT, move_penalty=0.5, u0=0.1 + 0.2 * u[0], du_max=0.05)
acid = wt.DMCLoop.from_fopdt("pH_inlet", 7.0 + 0.4 * u[1], -0.5, 100.0, 20.0, 2 * DT, horizon=24, move_penalty=1.0, every=2, u0=0.1)
blocks = wt.mpc_block(N, chlorine, acid)
idle = (wt.DMCLoop("chlorine_outlet", 1.0, [1.0], [0.1], enable=0), wt.DMCLoop("pH_inlet", 7.0, [-1.0], [-0.1], enable=0))

OUT = ("sensor_readings", "input_image", "boundary")

warm = plant(cols, bc, n)                                   # module load, first launches
warm.set_mpc(chlorine, acid); warm.step(DT, n_steps=2, download=False); warm.mpc_state(); warm.close()


def host_loop():
    ens = plant(cols, bc, n)
    ref = MpcRef(*blocks)
    ens.synchronize()
    t0 = time.perf_counter()
    HostScan(N, tun=LoopOwners(None, ref), emulated=True, dt=DT).run(ens, K, 1, fused=False, image=True)
    dt = time.perf_counter() - t0
    out = outputs(ens, *OUT)
    ens.close()
    return dt, out, (ref.st, ref.pred)


def fused(loops):
    ens = plant(cols, bc, n)
    if loops:
        ens.set_mpc(*loops)
    _, dt = timed_step(ens, DT, K)
    out = outputs(ens, *OUT)
    st = (ens.mpc_state().block(), ens.mpc_prediction()) if loops else None
    ens.close()
    return dt, out, st


ta, out_a, st_a = host_loop()
VARIANTS = {"mpc": (chlorine, acid), "none": None, "idle": idle}
times, median, last = rotate(tuple(VARIANTS), 5, lambda v, rep: fused(VARIANTS[v]))
tb, tc, td = median["mpc"], median["none"], median["idle"]
(_, out_b, st_b), (_, out_c, _), (_, out_d, _) = last["mpc"], last["none"], last["idle"]
equal, equal_idle = same(out_a, out_b) and same(st_a, st_b), same(out_c, out_d)
print(json.dumps({"N": N, "n": n, "steps": K, "host_loop_s": round(ta, 4), "fused_mpc_s": round(tb, 4),
                  "plant_io_only_s": round(tc, 4), "idle_mpc_s": round(td, 4), "loop_over_fused": round(ta / tb, 2),
                  "mpc_over_plant_io": round(tb / tc, 3), "idle_mpc_over_plant_io": round(td / tc, 3),
                  "fused_runs_s": {v: [round(t, 4) for t in ts] for v, ts in times.items()},
                  "executions": [int(st_b[0][l, 9].sum()) for l in range(2)],
                  "bitwise_equal": bool(equal), "idle_bitwise_equal_plant_io": bool(equal_idle)}))
if not (equal and equal_idle):
    sys.exit(1)
