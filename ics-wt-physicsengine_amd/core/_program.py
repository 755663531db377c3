"""What the per-reactor scan programs (:mod:`.control`, :mod:`.inject`, :mod:`.alarm`, :mod:`.actuator`) share on
the host: the sensor names, names -> codes, the rows of one loop or slot, and the packing of a slot program into its
block.  Each module keeps its own fields, defaults, off rows and ``validate_block``."""
from __future__ import annotations

import numpy as np

# the sensor suite's order: index = sensor code of every program block and row of ``sensor_readings``
SENSOR_NAMES = ("pH_inlet", "pH_outlet", "chlorine_inlet", "chlorine_outlet", "flow_main", "temp_inlet", "temp_outlet")


def codes(value, names, what) -> np.ndarray:
    """Names or indices -> float64 codes (validity is checked by the module's ``validate_block``)."""
    a = np.asarray(value)
    if a.dtype.kind in "US":
        bad = [s for s in a.ravel() if str(s) not in names]
        if bad:
            raise ValueError(f"unknown {what} {str(bad[0])!r}: one of {names}")
        return np.vectorize(lambda s: float(names.index(str(s))), otypes=[np.float64])(a)
    return a.astype(np.float64)


def field_rows(item, fields, n: int, name: str, **values) -> np.ndarray:
    """(len(fields), n) float64 rows of one loop or slot: each field of ``item`` (or its replacement in ``values``)
    broadcast to (n,)."""
    rows = np.empty((len(fields), n))
    for i, k in enumerate(fields):
        v = values[k] if k in values else getattr(item, k)
        try:
            rows[i] = np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))
        except ValueError:
            raise ValueError(f"{name}.{k}: expected a scalar or ({n},) values, got shape {np.shape(v)}") from None
    return rows


def slot_block(items, n: int, slots: int, what: str, rows_of, off_rows: np.ndarray, validate) -> np.ndarray:
    """The [slots][fields][n] float64 block of a slot program, validated: slot k holds ``rows_of(items[k], n, name)``,
    the slots after the last item hold ``off_rows``."""
    if len(items) > slots:
        raise ValueError(f"at most {slots} {what}s per program, got {len(items)}")
    rows = [rows_of(item, n, f"{what} {k}") for k, item in enumerate(items)]
    rows += [off_rows] * (slots - len(items))
    block = np.ascontiguousarray(np.stack(rows))
    validate(block)
    return block
