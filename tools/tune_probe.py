"""What relay autotuning with a scan per outer step costs, three ways, at 10 000 x 8 over 120 steps of 10 s:
  (a) the host loop it needs without the feature: step(dt, 1, fused=False), sensor_readings(), input_image(), the relay
      update in numpy (tests/tune_ref.py), write_holding(), every step;
  (b) one fused call with both tuners on the device (ReactorEnsemble.set_tuners), a scan per step;
  (c) the same call with plant I/O but no tuner, as the reference point;
  (d) the call of (b) with every experiment still waiting (a start beyond the run): the tuner runs but commands
      nothing, so the plant is (c)'s -- (d) over (c) is the waiting tuner's own cost.
Checks that (a) and (b) give bitwise the same states, readings, images, boundaries and tuner state, and (c) and (d) the
same plant, and prints one JSON line with the outcome counts of (b).
   python tools/tune_probe.py [N] [n] [steps]"""
import json, sys, time
import numpy as np
from probe_common import arguments, outputs, plant, same, timed_step, wt
from tune_ref import DONE, FAILED, RUNNING, US_PHASE, TuneRef
from program_helpers import HostScan

N, n, K, cols, bc = arguments(120)
DT = 10.0
u = np.random.default_rng(3).random((2, N))

# the setpoints: the outlet chlorine reading at 100 s, past the analyser's warm-up (the analysers carry a start-up offset)
first = plant(cols, bc, n)                                  # (also: module load, first launches)
first.step(DT, n_steps=10, download=False)
here = first.sensor_readings()[0][3].astype(np.float64)
first.close()
here = np.where(np.isfinite(here), here, np.nanmedian(here))


def tuners(start=0.0):
    chlorine = wt.RelayTune("chlorine_outlet", setpoint=here, amplitude=0.1 + 0.1 * u[0], bias=0.3, hysteresis=0.0, start=start,
                            timeout=0.75 * K * DT, settle=1, cycles=3)
    acid = wt.RelayTune("pH_outlet", setpoint=7.0 + 0.4 * u[1], amplitude=0.25, bias=0.5, direction=-1, start=start,
                        settle=0, cycles=2, rule="tyreus_luyben_pi")
    return chlorine, acid


block = wt.tune_block(N, *tuners())
OUT = ("sensor_readings", "input_image", "boundary")

warm = plant(cols, bc, n)                                   # module load, first launches
warm.set_tuners(*tuners()); warm.step(DT, n_steps=2, download=False); warm.tuner_state(); warm.close()


def host_loop():
    ens = plant(cols, bc, n)
    ref = TuneRef(block)
    ens.synchronize()
    t0 = time.perf_counter()
    HostScan(N, tun=ref, emulated=True, dt=DT).run(ens, K, 1, fused=False, image=True)
    dt = time.perf_counter() - t0
    out = outputs(ens, *OUT)
    ens.close()
    return dt, out, ref.st


def fused(tune):
    ens = plant(cols, bc, n)
    if tune:
        ens.set_tuners(*tune)
    _, dt = timed_step(ens, DT, K)
    out = outputs(ens, *OUT)
    st = ens.tuner_state().block() if tune else None
    ens.close()
    return dt, out, st


ta, out_a, st_a = host_loop()
tb, out_b, st_b = fused(tuners())
tc, out_c, _ = fused(None)
td, out_d, _ = fused(tuners(start=10.0 * K * DT))
equal, equal_idle = same(out_a, out_b) and np.array_equal(st_a, st_b, equal_nan=True), same(out_c, out_d)
phase = st_b[:, US_PHASE]
print(json.dumps({"N": N, "n": n, "steps": K, "host_loop_s": round(ta, 4), "fused_tune_s": round(tb, 4),
                  "plant_io_only_s": round(tc, 4), "waiting_tune_s": round(td, 4), "loop_over_fused": round(ta / tb, 2),
                  "tune_over_plant_io": round(tb / tc, 3), "waiting_tune_over_plant_io": round(td / tc, 3),
                  "done": [int((phase[l] == DONE).sum()) for l in range(2)], "failed": [int((phase[l] == FAILED).sum()) for l in range(2)],
                  "running": [int((phase[l] == RUNNING).sum()) for l in range(2)],
                  "bitwise_equal": bool(equal), "waiting_bitwise_equal_plant_io": bool(equal_idle)}))
if not (equal and equal_idle):
    sys.exit(1)
