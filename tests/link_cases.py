"""The scripted ensemble of the link-program tests (tests/test_link_cpu.py, tests/test_gpu_link.py): link slots of all
three modes on reading and command channels, the programs around them, and the host side of it all.  Times are in scans
of ``W`` seconds, so the same script serves a scan every step and every third.  ``SCANS`` = 80 scans wrap every ring
that records throughout.

The linked readings are the flow meter's and the inlet thermometer's: both instruments are past their warm-up by the
third scan and noisy from then on (the analysers and pH probes warm up for minutes), so a delayed or replayed image
differs from the field.  Both PI loops and the controller read the flow meter's image, so their words move with it.

Per reactor r:
  slot 0  flow meter.  r % 3 == 0: REPLAY of 4 scans in [20 W, 50 W) -- the IMAGE-against-FIELD detector (a CUSUM of
          image minus field) fires inside it.  r % 3 == 1: DELAY of 0, 1 (+ jitter 0..2), 3 or 63 scans by (r // 3) % 4
          in [10 W, 60 W).  r % 3 == 2: LOSS with probability 0, 0.5 or 1 by (r // 3) % 3 in [10 W, 60 W), no timeout.
  slot 1  inlet thermometer.  even r: LOSS 1 in [30 W, 45 W) with a timeout of 4 W into fault code 3 -- reached at the
          window's fifth scan, and the BAD-cause response slot engages on it.  odd r: LOSS 0.5 with a timeout of 1000 W
          into fault code 2, never reached.
  slot 2  chlorine command.  r % 3 == 0: LOSS 1 in [40 W, 55 W), timeout 5 W, fail-safe 0.0625.  r % 3 == 1: DELAY 3
          throughout.  r % 3 == 2: REPLAY of 5 scans in [40 W, 60 W).
  slot 3  even r: acid command, DELAY 63 from the first scan on (a window that opens with the first sample).  odd r: the
          flow meter again, DELAY 1 in [15 W, 25 W): two slots chained on one channel.
An injection program biases the flow meter's image in [25 W, 35 W) (the same channel, after the link), halves the
chlorine command in [50 W, 65 W) and raises the inlet flow command by 2 from 30 W on: the plant is driven off while the
tape plays, so the field reading leaves the replayed image whatever the meter's noise (a meter inside its hysteresis
band reads flat, and a flat tape equals the field).  r % 4 == 3: a model predictive controller has the chlorine loop; elsewhere the PI.
"""
import numpy as np

import link_ref as LR
import mpc_ref as MR
import respond_ref as RR
from control_ref import ControlRef
from detect_ref import DetectRef
from inject_ref import InjectRef

MASTER = (0.5, 0.25, 6.0)      # acid, chlorine, inlet flow commands before any program writes
SCANS = 80
SEED = 0x5EED0123456789
FLOW, T_IN = 4, 5


class Scenario:
    def __init__(self, wt, N, W):
        self.wt, self.N, self.W = wt, N, float(W)
        r = np.arange(N)
        self.r = r
        W = self.W
        g, k = r % 3, r // 3
        inf = np.inf
        delay = np.choose(k % 4, [0.0, 1.0, 3.0, 63.0])
        s0 = wt.Link("flow_main", np.choose(g, [3, 1, 2]), start=np.choose(g, [20 * W, 10 * W, 10 * W]),
                     end=np.choose(g, [50 * W, 60 * W, 60 * W]), a=np.choose(g, [4.0, delay, np.choose(k % 3, [0.0, 0.5, 1.0])]),
                     b=np.where((g == 1) & (delay == 1.0), 2.0, 0.0))
        even = r % 2 == 0
        s1 = wt.Link("temp_inlet", "loss", start=np.where(even, 30 * W, 0.0), end=np.where(even, 45 * W, inf),
                     a=np.where(even, 1.0, 0.5), timeout=np.where(even, 4 * W, 1000 * W), fail=np.where(even, 3.0, 2.0))
        s2 = wt.Link("chlorine_flow_rate", np.choose(g, [2, 1, 3]), start=np.choose(g, [40 * W, 0.0, 40 * W]),
                     end=np.choose(g, [55 * W, inf, 60 * W]), a=np.choose(g, [1.0, 3.0, 5.0]),
                     timeout=np.where(g == 0, 5 * W, inf), fail=np.where(g == 0, 0.0625, 0.0))
        s3 = wt.Link(np.where(even, 7, FLOW), "delay", start=np.where(even, 0.0, 15 * W), end=np.where(even, inf, 25 * W),
                     a=np.where(even, 63.0, 1.0))
        self.links = [s0, s1, s2, s3]
        self.script = [wt.Injection("flow_main", "bias", start=25 * W, end=35 * W, a=0.5),
                       wt.Injection("chlorine_flow_rate", "gain", start=50 * W, end=65 * W, a=0.5),
                       wt.Injection("inlet_flow_rate", "bias", start=30 * W, a=2.0)]
        self.replayed = g == 0
        self.attack = (np.where(self.replayed, 20 * W, inf), np.where(self.replayed, 50 * W, inf))
        self.detectors = [wt.Detector("flow_main", "cusum", limit=4.0, sigma=1e-3, ref="flow_main", ref_source="field", source="image")]
        self.pi = (wt.PILoop("flow_main", setpoint=6.0, kp=0.25 + 0.125 * (r % 2), ki=1.0 / 1024.0, bias=0.25),
                   wt.PILoop("flow_main", setpoint=6.5, kp=0.5, ki=1.0 / 2048.0, direction=-1, bias=0.5))
        self.dmc = wt.DMCLoop("flow_main", 6.0, step=[4.0], gain=[0.0625], horizon=1, u0=0.25, enable=(r % 4 == 3).astype(float))
        self.responses = [wt.Response("bad", "temp_inlet", "acid", action="manual", value=0.75, clear_delay=W)]
        self.blocks = dict(link=wt.link_block(N, *self.links), inject=wt.injection_block(N, *self.script),
                           detect=wt.detector_block(N, *self.detectors), control=wt.control_block(N, *self.pi),
                           mpc=wt.mpc_block(N, self.dmc), respond=wt.response_block(N, *self.responses))
        self.labels = np.stack([np.broadcast_to(np.asarray(a, dtype=np.float64), (N,)) for a in self.attack])

    def device(self, ens, link=True):
        """The programs on an ensemble with plant I/O: the link program (``link``), the injection script, the detector,
        the PI loops, the controller and the response program."""
        ens.write_commands(*MASTER)
        if link:
            ens.set_links(*self.links, seed=SEED)
        ens.set_injections(*self.script)
        ens.set_detectors(*self.detectors, attack=self.attack)
        ens.enable_control(*self.pi)
        ens.set_mpc(chlorine=self.dmc)
        ens.set_responses(*self.responses)

    def host(self, HostScan, words, dt, stepped=None, reactor_base=0):
        """The restatements of everything ``device`` sets, in a ``HostScan`` whose command path is emulated (the host
        master writes what the link and the injection leave of its words): (scan, refs by name)."""
        N, b = self.N, self.blocks
        ctl = ControlRef(b["control"], np.zeros(N), holding=words(np.array(MASTER)[:, None] * np.ones(N)))
        mpc = MR.MpcRef(*b["mpc"], words=ctl)
        det = DetectRef(b["detect"], self.labels, np.zeros(N))
        rsp = RR.RespondRef(b["respond"], np.zeros(N), words=ctl, ctl=ctl, mpc=mpc, det=det)
        lnk = LR.LinkRef(b["link"], seed=SEED, reactor_base=reactor_base)
        inj = InjectRef(b["inject"])
        hs = HostScan(N, ctl=ctl, tun=RR.ResponseOwners(None, rsp, mpc), inj=LR.LinkThenInject(lnk, inj, stepped), det=det,
                      emulated=True, dt=dt)
        return hs, dict(ctl=ctl, mpc=mpc, det=det, rsp=rsp, lnk=lnk, inj=inj)


def not_vacuous(params, state, what):
    """From a link program's own state (4, 10, N) and parameters (4, 8, N): each mode was applied on a reading and on a
    command channel, something was lost, a timeout occurred and one did not, and a ring wrapped."""
    mode, command = params[:, LR.L_MODE], params[:, LR.L_TARGET] >= LR.CMD_ACID
    applied = state[:, LR.LS_N_APPLIED] > 0
    for m, name in ((LR.DELAY, "delay"), (LR.LOSS, "loss"), (LR.REPLAY, "replay")):
        for kind in (False, True):
            assert (applied & (mode == m) & (command == kind)).any(), (what, name, "command" if kind else "reading", "never applied")
    assert state[:, LR.LS_N_LOST].any(), (what, "nothing was lost")
    lossy = (mode == LR.LOSS) & np.isfinite(params[:, LR.L_TIMEOUT])
    assert (lossy & (state[:, LR.LS_N_TIMEOUT] > 0)).any(), (what, "no timeout occurred")
    assert (lossy & (state[:, LR.LS_N_LOST] > 0) & (state[:, LR.LS_N_TIMEOUT] == 0)).any(), (what, "every timeout was reached")
    assert (state[:, LR.LS_N_REC] > LR.DEPTH).any(), (what, "no ring wrapped")
    assert (state[:, LR.LS_N_DRAW] > 0).any() and ((mode == LR.DELAY) & (params[:, LR.L_B] > 0) & applied).any(), (what, "no jitter")
