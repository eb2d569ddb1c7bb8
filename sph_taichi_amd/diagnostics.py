"""Flow diagnostics: what `ParticleSystem.diagnostics()` returns (include/sph_hip.h, last section; csrc/sph_diag.hip).

The reference's older engine learns max |v|, max |a|, max density and max pressure from whole-array `to_numpy()` copies
every step (legacy/engine/sph_solver.py:712-761); here one streaming reduction on the device leaves one row per object
and one over all particles, and only those rows cross to the host.  Nothing in this module touches the GPU when it is
imported: the library is reached through the ParticleSystem handed to `reduce`.
"""
from __future__ import annotations

import math

_RAW_SCALARS = ("count", "fluid_count", "moving_count", "mass", "kinetic", "v2_max", "a2_max", "density_min",
                "density_max", "pressure_min", "pressure_max")
_RAW_VECTORS = ("mx", "momentum", "lo", "hi")


class DiagRow:
    """One row of the reduction: the raw members of `SphDiagRow` (Python ints / floats / 3-tuples) and what follows from
    them.  `g` is the scene's gravitation."""

    def __init__(self, raw, g=(0.0, -9.81, 0.0)):
        for k in _RAW_SCALARS:
            v = getattr(raw, k)
            setattr(self, k, int(v) if k.endswith("count") else float(v))
        for k in _RAW_VECTORS:
            setattr(self, k, tuple(float(v) for v in getattr(raw, k)))
        self.g = tuple(float(v) for v in g)

    @property
    def v_max(self) -> float:
        return math.sqrt(self.v2_max)

    @property
    def a_max(self) -> float:
        return math.sqrt(self.a2_max)

    @property
    def center_of_mass(self):
        """mx / mass; None for a row without mass."""
        return tuple(c / self.mass for c in self.mx) if self.mass != 0.0 else None

    @property
    def potential(self) -> float:
        """-g . sum m x (zero level at the origin)."""
        return -sum(gc * c for gc, c in zip(self.g, self.mx))

    @property
    def energy(self) -> float:
        return self.kinetic + self.potential

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k in _RAW_SCALARS}
        d.update({k: list(getattr(self, k)) for k in _RAW_VECTORS})
        com = self.center_of_mass
        d.update(v_max=self.v_max, a_max=self.a_max, center_of_mass=list(com) if com is not None else None,
                 potential=self.potential, energy=self.energy)
        return d


class Diagnostics:
    """`time` = the context's clock when the rows were reduced, `total` = all particles, `objects[object_id]` = one object."""

    def __init__(self, time: float, objects, total: DiagRow):
        self.time = float(time)
        self.objects = list(objects)
        self.total = total

    def as_dict(self) -> dict:
        return {"time": self.time, "total": self.total.as_dict(), "objects": [r.as_dict() for r in self.objects]}


def download_rows(ps):
    """sph_diag_reduce + sph_diag_download: the raw `SphDiagRow` array (n_objects + 1 rows; synchronises)."""
    from . import _lib
    n_rows = int(ps._params.n_objects) + 1
    rows = (_lib.SphDiagRow * n_rows)()
    ps._call("sph_diag_reduce")
    ps._call("sph_diag_download", rows, n_rows)
    return rows


def reduce(ps) -> Diagnostics:
    if ps.slab is not None:
        raise NotImplementedError("diagnostics exist on single-domain contexts only: a slab rank's ghost records would be "
                                  "counted twice (the rows of the ranks' owned ranges would have to be all-reduced)")
    g = ps.cfg.get_cfg("gravitation") or [0.0, -9.81, 0.0]
    rows = download_rows(ps)
    made = [DiagRow(r, g) for r in rows]
    return Diagnostics(ps.time, made[:-1], made[-1])
