"""The installation of the fused sensor suite (include/wtphys.h, ``wt_ensemble_install_*``): every reactor's own
sample lines and instrument installation.

``create_realistic_sensor_suite`` builds one fixed installation -- two 250 mL sample lines at 500 mL/min (30 s of dead
time) and one ``InstallationQuality`` for all seven sensors -- and that is what an ensemble computes while no
installation is set.  The reference models both per sensor object: a ``SampleLine`` whose delay is its volume over its
flow, and the installation branches of ``BaseSensor._apply_installation_effects`` (stagnant flow, air bubbles, poor
grounding, vibration), the stagnant ageing rates of the pH electrode and the amperometric cell, the flowmeter's bubble
dropouts and the RTD's stem error against the ambient temperature.  This module builds the parameter block; the
library checks it (``wt_install_check``), derives the delays, and the reads run in ``csrc/wt_sensors.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Union

import numpy as np

from . import _native
from ._program import field_rows

NINS = 9                                   # WT_NINS
PARAM_ROWS = ("inlet_line_volume_mL", "inlet_line_flow_mL_min", "outlet_line_volume_mL", "outlet_line_flow_mL_min",
              "flow_velocity", "air_bubble_frequency", "grounding_quality", "pipe_vibration_g", "ambient_temperature")

Value = Union[float, int, np.ndarray]


@dataclass
class Installation:
    """One installation per reactor; every field takes a scalar or an (N,) array, and the defaults are the suite's
    own build.  The inlet line is the ``SampleLine`` that pH_inlet and temp_inlet share, the outlet line that of
    pH_outlet and temp_outlet: delay = (volume / 1000) / (flow / 1000 / 60) seconds, 0 for a flow of 0, below 91 s (the
    reference's 100-entry buffer).  The other five fields are the one ``InstallationQuality`` of all seven sensors:
    ``flow_velocity`` [m/s] below 0.1 adds stagnant scatter and speeds up pH scaling and amperometric fouling;
    ``air_bubble_frequency`` [1/min] above 0 makes a read NaN with probability frequency / 60 -- for good, since the
    reference's lag keeps the NaN -- and drops flowmeter reads to 0.0; ``grounding_quality`` below 0.8 and
    ``pipe_vibration_g`` above 0.2 add noise; ``ambient_temperature`` [degC] enters the RTDs' stem error.

    ``SampleLine.ambient_temp`` has no field: the reference computes the cooled sample temperature and throws it away
    (base_sensor.py:611-614), so no reading depends on it."""

    inlet_line_volume_mL: Value = 250.0
    inlet_line_flow_mL_min: Value = 500.0
    outlet_line_volume_mL: Value = 250.0
    outlet_line_flow_mL_min: Value = 500.0
    flow_velocity: Value = 0.5
    air_bubble_frequency: Value = 0.0
    grounding_quality: Value = 0.9
    pipe_vibration_g: Value = 0.1
    ambient_temperature: Value = 30.0


def check(block: np.ndarray) -> None:
    """The checks ``wt_ensemble_install_set`` makes on a C-contiguous float64 (NINS, N) block; ``ValueError`` names the
    first one that fails."""
    try:
        _native.check(_native.lib().wt_install_check(block.shape[-1], _native.dptr(block)))
    except _native.WtError as e:   # WT_E_ARG is the only error it returns
        raise ValueError(e.message) from None


def installation_block(n_reactors: int, inst: Optional[Installation] = None) -> np.ndarray:
    """The [WT_NINS][N] float64 block of ``wt_ensemble_install_set``, checked by the library; without ``inst`` the
    suite's own build for every reactor."""
    if inst is None:
        inst = Installation()
    if not isinstance(inst, Installation):
        raise TypeError(f"installation: expected an Installation, got {type(inst).__name__}")
    block = np.ascontiguousarray(field_rows(inst, PARAM_ROWS, int(n_reactors), "installation"))
    check(block)
    return block
