"""The sensor service program (include/wtphys.h, ``wt_ensemble_service_*``): calibrate, clean and replace the
instruments of the fused sensor suite on a schedule, inside the step call.

The reference's sensors have a maintenance interface next to ``read`` -- ``calibrate``, ``calibrate_two_point``,
``clean_electrode``, ``replace_membrane``, ``replace_reagent`` -- which its loop would call between two iterations.
A program has up to four slots per reactor.  A slot names one sensor and one action and falls due either at a suite
time (once, or every ``every`` seconds) or some time after a read of its sensor returned a given status; the action
then acts on the next read.  This module builds the parameter block and unpacks the state; the library checks the
block (``wt_program_check``), and the actions themselves run in ``csrc/wt_svc.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Union

import numpy as np

from . import _native
from ._program import SENSOR_NAMES, codes, field_rows, slot_block

SLOTS, NSV, NSVS, NSH = 4, 12, 4, 8       # WT_SVC_SLOTS, WT_NSV, WT_NSVS, WT_NSH
PARAM_ROWS = ("enable", "sensor", "action", "trigger", "t_first", "period", "count", "status", "delay", "ref_mode", "ref", "ref2")
STATE_ROWS = ("n_done", "t_last", "t_due", "t_seen")
HEALTH_ROWS = ("cal_offset", "cal_time", "power_on", "slow0", "slow1", "slow2", "status", "fault")
ACTIONS = ("calibrate", "two_point", "rinse", "acid_clean", "pepsin_clean", "replace_membrane", "replace_reagent")
TRIGGERS = ("at_time", "on_status")
REF_MODES = ("constant", "sample", "trim")
# SensorStatus in declaration order (sensors/base_sensor.py:49-62): the codes of ``sensor_readings()[1]``
STATUS_NAMES = ("normal", "calibrating", "warming_up", "failed", "saturated", "drift_warning", "cal_expired", "open_circuit",
                "short_circuit", "out_of_range", "power_fault", "rate_fault")

Value = Union[float, int, str, np.ndarray]


@dataclass
class Service:
    """One slot.  ``sensor``: a name of :data:`SENSOR_NAMES` or its index; ``action``: one of :data:`ACTIONS`.
    Trigger, one of the two: ``at`` -- due once the suite time (seconds since ``enable_sensors``) reaches it, then
    every ``every`` seconds (0: once); ``on_status`` -- a name of :data:`STATUS_NAMES` or its code: the first read of
    the sensor that returns it writes a work order, which is carried out ``delay`` seconds later whether or not the
    status has cleared.  ``count`` caps the slot's services (0: no cap).  ``ref_mode``: the calibration's reference
    value is ``ref`` ("constant"), the true value at the sensor's tap plus ``ref`` ("sample": a grab sample with a
    bias), or that plus the offset in force ("trim": what removes an old offset, since the reference's ``calibrate``
    replaces the offset instead of accumulating it).  "two_point" takes the buffers ``ref`` and ``ref2``; the replace
    actions calibrate against the reference's fixed 0.0.  Every field takes a scalar or an (N,) array."""

    sensor: Value
    action: Value
    at: Optional[Value] = None
    every: Value = 0.0
    count: Value = 0
    on_status: Optional[Value] = None
    delay: Value = 0.0
    ref: Value = 0.0
    ref2: Value = 0.0
    ref_mode: Value = "constant"


@dataclass
class ServiceState:
    """``ReactorEnsemble.service_state()``: (SLOTS, N) float64 each."""

    n_done: np.ndarray         # services the slot has carried out
    t_last: np.ndarray         # suite time of the last one (NaN: none yet)
    t_due: np.ndarray          # at_time slots: the suite time of the next service (+inf: none left)
    t_seen: np.ndarray         # on_status slots: suite time the work order was written (NaN: none open)

    @classmethod
    def from_block(cls, block: np.ndarray) -> "ServiceState":
        """From a [WT_SVC_SLOTS][WT_NSVS][N] block."""
        return cls(*(np.array(block[:, k]) for k in range(NSVS)))

    def block(self) -> np.ndarray:
        """The (SLOTS, NSVS, N) block again."""
        return np.stack([getattr(self, k) for k in STATE_ROWS], axis=1)


def slot_rows(service: Service, n: int, name: str = "service") -> np.ndarray:
    """(NSV, N) rows of one slot."""
    if not isinstance(service, Service):
        raise TypeError(f"{name}: expected a Service, got {type(service).__name__}")
    if (service.at is None) == (service.on_status is None):
        raise ValueError(f"{name}: give either at= (a suite time) or on_status= (a status), not both or neither")
    timed = service.on_status is None
    return field_rows(service, PARAM_ROWS, n, name, enable=1.0, sensor=codes(service.sensor, SENSOR_NAMES, "sensor"),
                      action=codes(service.action, ACTIONS, "action"), trigger=0.0 if timed else 1.0,
                      t_first=service.at if timed else 0.0, period=service.every,
                      status=0.0 if timed else codes(service.on_status, STATUS_NAMES, "status"),
                      ref_mode=codes(service.ref_mode, REF_MODES, "ref_mode"))


def service_block(n_reactors: int, *services: Service) -> np.ndarray:
    """The [WT_SVC_SLOTS][WT_NSV][N] float64 block of ``wt_ensemble_service_set``, checked by the library: slot k is
    the k-th service, the slots after the last are off."""
    n = int(n_reactors)
    return slot_block(services, n, SLOTS, "service", slot_rows, np.zeros((NSV, n)), _native.WT_PROG_SERVICE)
