"""Solver adapters (same call signatures as ``pockit.optimizer``): ``ipopt`` (needs cyipopt and Ipopt) and ``scipy``
(``trust-constr`` through the host callbacks) -- and ``interior_point``, this package's own primal-dual interior-point solver on
its device-resident units, which needs no third-party optimiser: ``interior_point.solve(system, guess)``."""
