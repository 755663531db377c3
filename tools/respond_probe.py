"""What a response program with a scan per outer step costs, three ways, at 10 000 x 8 over 120 steps of 10 s:
  (a) the host loop it needs without the feature: step(dt, 1, fused=False), sensor_readings(), input_image(), the PI,
      alarm, detector and response programs in numpy (tests/control_ref.py, alarm_ref.py, detect_ref.py,
      respond_ref.py), write_holding(), every step;
  (b) one fused call with all four programs on the device, a scan per step;
  (c) the same call without the response program, as the reference point.
Every reactor has one detector-caused slot (a CUSUM on the outlet analyser in alarm: hold the chlorine dose, hand back
bumpless after two clear scans) and one alarm-caused slot (outlet chlorine above a per-reactor limit for 20 s: drive the
acid dose to 0.25 by hand, at least 60 s).  The limits lie around the initial chlorine, so the plant's own noise and
drift raise the causes in a good part of the ensemble; the JSON line's engagement counts say in how many.  Checks that
(a) and (b) give bitwise the same states, readings, images, boundaries and program states, and prints one JSON line.  The
two fused calls run five times each in rotating order and report their medians, every run is listed, and the host loop
runs once.  Times are reported, nothing is asserted about them.
   python tools/respond_probe.py [N] [n] [steps]"""
import json, sys, time
import numpy as np
from probe_common import arguments, outputs, pi_loops, plant, rotate, same, timed_step, wt
from alarm_ref import AlarmRef
from control_ref import ControlRef
from detect_ref import DetectRef
from respond_ref import RS_N_ENGAGED, RS_N_HANDBACK, RS_N_OWNED, RespondRef, ResponseOwners
from program_helpers import HostScan

N, n, K, cols, bc = arguments(120)
DT = 10.0
chlorine, acid, u = pi_loops(cols, N, rows=6)
cl0 = np.asarray(cols["initial_chlorine"])
alarm = wt.Alarm("chlorine_outlet", "high", cl0 - 0.05 + 0.1 * u[4], deadband=0.01)
detector = wt.Detector("chlorine_outlet", "cusum", limit=4.0 + 4.0 * u[5], sigma=0.02, ref_value=cl0)
slots = (wt.Response("detector", 0, "chlorine", action="hold", handback="bumpless", clear_delay=2 * DT),
         wt.Response("alarm", 0, "acid", action="manual", value=0.25, delay=2 * DT, min_hold=6 * DT))
blocks = dict(control=wt.control_block(N, chlorine, acid), alarm=wt.alarm_block(N, alarm), detect=wt.detector_block(N, detector),
              respond=wt.response_block(N, *slots))

OUT = ("sensor_readings", "input_image", "boundary")

warm = plant(cols, bc, n)                                   # module load, first launches
warm.set_responses(*slots); warm.step(DT, n_steps=2, download=False); warm.response_state(); warm.close()


def programs(ens):
    ens.enable_control(chlorine, acid)
    ens.set_alarms(alarm)
    ens.set_detectors(detector)


def host_loop():
    ens = plant(cols, bc, n)
    ctl = ControlRef(blocks["control"], np.zeros(N))
    alm, det = AlarmRef(blocks["alarm"], np.zeros(N)), DetectRef(blocks["detect"], np.full((2, N), np.inf), np.zeros(N))
    rsp = RespondRef(blocks["respond"], np.zeros(N), words=ctl, ctl=ctl, alm=alm, det=det)
    ens.synchronize()
    t0 = time.perf_counter()
    HostScan(N, ctl=ctl, tun=ResponseOwners(None, rsp), alm=alm, det=det, emulated=True, dt=DT).run(ens, K, 1, fused=False, image=True)
    dt = time.perf_counter() - t0
    out = outputs(ens, *OUT)
    ens.close()
    return dt, out, (ctl.st, alm.st, det.st, rsp.st, rsp.rst)


def fused(respond):
    ens = plant(cols, bc, n)
    programs(ens)
    if respond:
        ens.set_responses(*slots)
    _, dt = timed_step(ens, DT, K)
    out = outputs(ens, *OUT)
    st = None
    if respond:
        st = (ens.control_state().block(), ens.alarm_state().block()[0], ens.detector_state().block()[0]) + tuple(ens.response_state().block())
    ens.close()
    return dt, out, st


ta, out_a, st_a = host_loop()
times, median, last = rotate(("respond", "none"), 5, lambda v, rep: fused(v == "respond"))
tb, tc = median["respond"], median["none"]
(_, out_b, st_b), _ = last["respond"], last["none"]
equal = same(out_a, out_b) and same(st_a, st_b)
rs = st_b[3]
print(json.dumps({"N": N, "n": n, "steps": K, "host_loop_s": round(ta, 4), "fused_respond_s": round(tb, 4),
                  "without_respond_s": round(tc, 4), "loop_over_fused": round(ta / tb, 2), "respond_over_without": round(tb / tc, 3),
                  "fused_runs_s": {v: [round(t, 4) for t in ts] for v, ts in times.items()},
                  "reactors_engaged": [int((rs[s, RS_N_ENGAGED] > 0).sum()) for s in range(2)],
                  "scans_owned": [int(rs[s, RS_N_OWNED].sum()) for s in range(2)],
                  "bumpless_handbacks": int(rs[:, RS_N_HANDBACK].sum()), "bitwise_equal": bool(equal)}))
if not equal:
    sys.exit(1)
