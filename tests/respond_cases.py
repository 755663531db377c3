"""The scripted ensemble of the response-program tests (tests/test_respond_cpu.py, tests/test_gpu_respond.py) and of
tools/respond_probe.py: injection windows that script every cause, the programs around the response program, and the
host side of it all.  Times are in scans of ``W`` seconds, so the same script serves a scan every step and every third.

The causes do not depend on the physics.  An injection program holds the outlet chlorine reading at LOW and, in a
window, at HIGH: the alarm slot (a HIGH limit between the two) is active from the window's first scan to the first
scan after it, and the detector slot (a CUSUM on the same reading) is in alarm from the window's first scan on and for
eight scans after its end; the response program sees both one scan later.  A drop-out window on the flow meter
and a fault-code window on the inlet thermometer are BAD causes in the scan that sees them (both instruments are past
their warm-up by the third scan; the analysers and pH probes are not for minutes).

Per reactor r:
  slot 0  alarm 0 -> chlorine, MANUAL 0.125, bumpless, clear_delay 2 scans, delay 0, 1, 3 or 8 scans or +inf by r % 5
          (the cause stands for five scans: the last two are never reached);
  slot 1  detector 0 -> chlorine, HOLD, bump, delay 0 or 2 scans, min_hold 16 scans where r % 3 == 0; off where
          r % 8 is 4 or 7.  While slot 0 is engaged it is outranked and tracks; it takes the loop over when slot 0 lets go;
  slot 2  flow meter BAD -> acid, RAMP to 0.75 at 1/128 per second, bumpless, delay 0 or 1 scan, clear_delay 1 scan;
  slot 3  inlet thermometer BAD -> acid, MANUAL 0.5 (even r) or HOLD, delay 3 scans (longer than the thermometer's
          warm-up), latched where r % 3 == 0.
  r % 4 == 2: a relay experiment on the chlorine loop from scan 8 on that fails after nine scans -- slots 0 and 1 are
              blocked meanwhile;
  r % 4 == 3: a model predictive controller has the chlorine loop; elsewhere the chlorine PI.  The acid PI's probe is
              in its warm-up throughout: a bumpless hand-back to it takes the branch of an invalid reading.
"""
import numpy as np

import mpc_ref as MR
import respond_ref as RR
import tune_ref as UR
from alarm_ref import AlarmRef
from control_ref import ControlRef
from detect_ref import DetectRef
from inject_ref import InjectRef

LOW, HIGH, LIMIT = 1.25, 2.0, 1.5
MASTER = (0.5, 0.25, 6.0)      # acid, chlorine, inlet flow commands before any program writes
SCANS = 48                     # a run of the script: every release has happened by then


class Scenario:
    def __init__(self, wt, N, W):
        self.wt, self.N, self.W = wt, N, float(W)
        r = np.arange(N)
        self.r = r
        W = self.W
        a0 = W * (10 + r % 3)
        self.script = [wt.Injection("chlorine_outlet", "constant", start=0.0, end=np.inf, a=LOW),
                       wt.Injection("chlorine_outlet", "constant", start=a0, end=a0 + 5 * W, a=HIGH),
                       wt.Injection("flow_main", "dropout", start=W * (6 + r % 2), end=W * (14 + r % 2)),
                       wt.Injection("temp_inlet", "fault", start=W * 20, end=W * 26, a=3)]
        self.attack = (a0, a0 + 5 * W)
        self.alarms = [wt.Alarm("chlorine_outlet", "high", LIMIT, deadband=0.125)]
        self.detectors = [wt.Detector("chlorine_outlet", "cusum", limit=1.5, slack=1.0, sigma=0.25, ref_value=LOW)]
        self.pi = (wt.PILoop("chlorine_outlet", setpoint=LIMIT, kp=0.5 + 0.25 * (r % 2), ki=1.0 / 1024.0, bias=0.25),
                   wt.PILoop("pH_outlet", setpoint=7.2, kp=0.4, ki=5e-4, direction=-1, bias=0.125))
        self.tune = wt.RelayTune("chlorine_outlet", setpoint=LIMIT, amplitude=0.125, bias=0.375, start=8 * W, timeout=9 * W,
                                 settle=0, cycles=1, enable=(r % 4 == 2).astype(float))
        self.dmc = wt.DMCLoop("chlorine_outlet", LIMIT, step=[4.0], gain=[0.0625], horizon=1, u0=0.25,
                              enable=(r % 4 == 3).astype(float))
        self.responses = [
            wt.Response("alarm", 0, "chlorine", action="manual", value=0.125, handback="bumpless", clear_delay=2 * W,
                        delay=np.choose(r % 5, [0.0, W, 3 * W, 8 * W, np.inf])),
            wt.Response(np.where((r % 8 == 4) | (r % 8 == 7), "off", "detector"), 0, "chlorine", action="hold",
                        delay=np.where((r // 2) % 2 == 0, 0.0, 2 * W), min_hold=np.where(r % 3 == 0, 16 * W, 0.0)),
            wt.Response("bad", "flow_main", "acid", action="ramp", value=0.75, rate=1.0 / 128.0, handback="bumpless",
                        delay=W * (r % 2), clear_delay=W),
            wt.Response("bad", "temp_inlet", "acid", action=np.where(r % 2 == 0, "manual", "hold"), value=0.5,
                        delay=3 * W, latch=(r % 3 == 0).astype(float))]
        self.blocks = dict(inject=wt.injection_block(N, *self.script), alarm=wt.alarm_block(N, *self.alarms),
                           detect=wt.detector_block(N, *self.detectors), control=wt.control_block(N, *self.pi),
                           tune=wt.tune_block(N, self.tune), mpc=wt.mpc_block(N, self.dmc),
                           respond=wt.response_block(N, *self.responses))
        self.labels = np.stack([np.broadcast_to(np.asarray(a, dtype=np.float64), (N,)) for a in self.attack])

    def device(self, ens, respond=True, around=True):
        """The programs on an ensemble with plant I/O: the script, the alarm and detector programs, then (``around``)
        the PI loops, the relay and the controller, then (``respond``) the response program."""
        ens.write_commands(*MASTER)
        ens.set_injections(*self.script)
        if around:
            ens.set_alarms(*self.alarms)
            ens.set_detectors(*self.detectors, attack=self.attack)
            ens.enable_control(*self.pi)
            ens.set_tuners(self.tune)
            ens.set_mpc(chlorine=self.dmc)
        if respond:
            ens.set_responses(*self.responses)

    def host(self, HostScan, words, dt):
        """The restatements of everything ``device`` sets, in a ``HostScan``: (scan, refs by name)."""
        N, b = self.N, self.blocks
        ctl = ControlRef(b["control"], np.zeros(N), holding=words(np.array(MASTER)[:, None] * np.ones(N)))
        tun = UR.TuneRef(b["tune"], ctl=ctl)
        mpc = MR.MpcRef(*b["mpc"], words=ctl)
        alm, det = AlarmRef(b["alarm"], np.zeros(N)), DetectRef(b["detect"], self.labels, np.zeros(N))
        rsp = RR.RespondRef(b["respond"], np.zeros(N), words=ctl, ctl=ctl, mpc=mpc, alm=alm, det=det)
        hs = HostScan(N, ctl=ctl, tun=RR.ResponseOwners(tun, rsp, mpc), inj=InjectRef(b["inject"]), alm=alm, det=det, dt=dt)
        return hs, dict(ctl=ctl, tun=tun, mpc=mpc, alm=alm, det=det, rsp=rsp)


def not_vacuous(params, state, what):
    """From a response program's own state (4, 14, N) and parameters (4, 11, N): each action engaged and released at
    least once, some slot was blocked, some slot was outranked, some bumpless hand-back happened."""
    done = (state[:, RR.RS_N_ENGAGED] > 0) & ~np.isnan(state[:, RR.RS_T_RELEASED]) & (params[:, RR.R_CAUSE] != RR.OFF)
    for action, name in ((RR.HOLD, "hold"), (RR.MANUAL, "manual"), (RR.RAMP, "ramp")):
        assert (done & (params[:, RR.R_ACTION] == action) & (state[:, RR.RS_N_OWNED] > 0)).any(), (what, name, "never engaged, owned and released")
    assert state[:, RR.RS_N_BLOCKED].any(), (what, "no slot was blocked")
    assert state[:, RR.RS_N_TRACKED].any(), (what, "no slot was outranked")
    assert state[:, RR.RS_N_HANDBACK].any(), (what, "no bumpless hand-back")
