"""Host restatement of the wire program (include/wtphys.h ``wt_ensemble_wire_*``, csrc/wt_wir.hpp): the routing of one
PLC scan's readings along the signal cables of every train, its two counters, and the PLC scan with the routing in
front (``WireScan``).  The host loop -- a handle without the program, calls of one scan interval, ``sensor_readings()``
routed here and the scan programs run on the result as a host master -- is the definition; the fused call must give
its bits."""
import numpy as np

import trend_ref as TR
from program_helpers import HostScan
from train_ref import ST_T_RANGE_POST

NSENS, OWN, FL_OPEN_CIRCUIT = 7, -1, 1
W_STAGE, W_SENSOR = 0, 1


class WireRef:
    """``params``: the (7, 2, N) block of ``wire_block`` for trains of ``length`` stages; ``n_routed`` / ``n_lost``
    (7, N) as ``ReactorEnsemble.wire_state()`` gives them."""

    def __init__(self, params, length):
        self.p = np.array(params, dtype=np.float64)
        self.N, self.length = self.p.shape[2], int(length)
        self.n_routed = np.zeros((NSENS, self.N))
        self.n_lost = np.zeros((NSENS, self.N))

    def route(self, v, f, stepped=None):
        """One scan: readings ``v`` float32 (7, N) and fault codes ``f`` (7, N) as the instruments gave them ->
        the controller-side copies (vw, fw).  For every reactor in ``stepped`` (default: all) each wired slot gets
        sensor s of stage g of its own train from ``v`` / ``f`` themselves -- never from the copies, so wires do not
        chain -- or NaN / fault 1 where the source reactor did not step."""
        v = np.asarray(v, dtype=np.float32)
        f = np.asarray(f).astype(np.int64)
        stepped = np.ones(self.N, dtype=bool) if stepped is None else np.asarray(stepped, dtype=bool)
        vw, fw = v.copy(), f.copy()
        r = np.arange(self.N)
        first = r - r % self.length
        for i in range(NSENS):
            g, s = self.p[i, W_STAGE].astype(np.int64), self.p[i, W_SENSOR].astype(np.int64)
            wired = stepped & (g != OWN)
            src = np.where(wired, first + g, r)
            up = wired & stepped[src]
            lost = wired & ~stepped[src]
            vw[i] = np.where(up, v[s, src], np.where(lost, np.float32(np.nan), v[i]))
            fw[i] = np.where(up, f[s, src], np.where(lost, FL_OPEN_CIRCUIT, f[i]))
            self.n_routed[i] += up
            self.n_lost[i] += lost
        return vw, fw

    def state(self):
        """The (7, 2, N) block of ``WireState.block()``."""
        return np.stack([self.n_routed, self.n_lost], axis=1)


class WireScan(HostScan):
    """``HostScan`` with the routing at the head of the scan: route -> inject -> pack -> ... in the device's order.  The
    injection, the PI loops, the IMAGE slots and the trend recorder's image tags get the routed copies; alarms,
    detectors and the recorder's field tags keep the raw (v, f) as FIELD."""

    def __init__(self, N, wir, **kw):
        super().__init__(N, **kw)
        self.wir = wir

    def scan(self, v, f, cmd=None, stepped=None, tags=None):
        assert cmd is None or not self.emulated, "an emulated command path runs in holding()"
        t = self.lt
        vw, fw = (v, f) if self.wir is None else self.wir.route(v, f, stepped)
        vt, ft = (vw, fw) if self.inj is None else self.inj.sensors(vw, fw, t, stepped)
        if cmd is not None:
            cmd = self._command_path(cmd, stepped)
            if self.act is not None:
                self.act.scan(cmd, t, stepped)
        if self.ctl is not None:
            self.ctl.scan(vt, ft, t, stepped)
        if self.alm is not None:
            self.alm.scan(v, f, t, stepped, image=(vt, ft))
        if self.det is not None:
            self.det.scan(v, f, t, stepped, image=(vt, ft))
        if self.trd is not None:
            self.values = {**self.tag_values(v, f, vt, ft), **(tags or {})}
            self.trd.scan(self.values, t, stepped)
        return vt, ft


FROZEN = 1 | ST_T_RANGE_POST | 64     # T_RANGE, T_RANGE_POST, NONFINITE: a reactor with one of them takes no further step


def took_the_step(status):
    """(N,) bool: the reactors whose readings the last outer step of a call refreshed -- they stepped and did not end
    T_RANGE_POST (the sensor suite's test).  A reactor that stops stays stopped, so the status after the call says it."""
    return (np.asarray(status) & FROZEN) == 0


def host_wired_loop(ens, hs, n_steps, interval, fused=True, commands_of=None):
    """The host loop a fused call with a wire program replaces, on a handle WITHOUT the wire program and without the
    scan programs that ``hs`` (a ``WireScan``) restates: calls of one scan interval, each after the master's write of
    ``hs.holding()`` and closed by ``hs.scan`` of ``sensor_readings()``.  ``commands_of(words)``: the decoded commands
    for a scan that is not ``emulated``.  Returns, per reactor, what the last scan it took part in saw: image values
    (7, N), image faults (7, N) and the loop time its input image holds (N,; NaN: it never took part)."""
    N = ens.n_reactors
    seen_v, seen_f, seen_t = np.full((NSENS, N), np.nan, dtype=np.float32), np.zeros((NSENS, N), dtype=np.int64), np.full(N, np.nan)
    for c in hs.calls(n_steps, interval):
        w = hs.holding()
        ens.write_holding(w)
        ens.step(hs.dt, n_steps=c, fused=fused, download=False)
        stepped = took_the_step(ens.status())
        v, _, f = ens.sensor_readings()
        tags = None if hs.trd is None else {TR.COMMAND: ens.boundary()[[4, 6, 0]]}
        vt, ft = hs.scan(v, f, None if hs.emulated else commands_of(w), stepped=stepped, tags=tags)
        seen_v[:, stepped], seen_f[:, stepped] = np.asarray(vt)[:, stepped], np.asarray(ft)[:, stepped]
        seen_t[stepped] = (hs.lt - hs.dt)[stepped]
    return seen_v, seen_f, seen_t
