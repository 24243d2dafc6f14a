"""The merit terms of a batch of trial points as the device reduces them (csrc/pk_merit.cpp): column names and the small
read-only result ``System.merit_batch`` / ``System.merit_scan`` return."""
from __future__ import annotations

import numpy as np

COLUMNS = ("f", "theta1", "theta_inf", "theta2_sq", "bound1", "bound_inf", "slope", "bad")


class MeritTable:
    """``(B, 8)`` merit terms, one row per trial point, read-only: ``table`` is the array, every name of ``COLUMNS`` a
    ``(B,)`` view of its column."""

    __slots__ = ("table",)

    def __init__(self, table):
        table = np.array(table, dtype=np.float64).reshape(-1, len(COLUMNS))
        table.flags.writeable = False
        object.__setattr__(self, "table", table)

    def __setattr__(self, name, value):
        raise AttributeError("a MeritTable is read-only")

    def __len__(self):
        return self.table.shape[0]

    def __repr__(self):
        return f"MeritTable({self.table.shape[0]} points; columns {', '.join(COLUMNS)})"


for _q, _name in enumerate(COLUMNS):
    setattr(MeritTable, _name, property(lambda self, _q=_q: self.table[:, _q]))
