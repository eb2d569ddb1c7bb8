"""ParticleSystem with the reference's attribute / method surface
(/root/reference/particle_system.py:10-495), backed by a HIP context.

What stays on the host (NumPy): scene ingestion (sph_taichi_amd/scene.py).
What moved to the GPU: every per-particle array (owned by libsph_hip's context,
exposed here as DeviceField objects with the reference's names) and the
neighbour-structure kernels update_grid_id / prefix sum / counting_sort.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, motion as _motion, scene as _scene
from .config_builder import SimConfig
from .field import DeviceField, HostScalar


class ParticleSystem:
    def __init__(self, config: SimConfig, GGUI=False, device: int = 0, stream=None, scene_dir: str | None = None,
                 verbose: bool = False, slab: dict | None = None, populate: bool = True, state: dict | None = None):
        """`slab` (multi-GPU, no reference counterpart) = dict(x_lo, x_hi, halo, capacity[, nx_slack]): this
        context owns the global cell layers [x_lo, x_hi) plus `halo` ghost layers on each side; `nx_slack` more
        layers are allocated so that a re-cut (`set_slab_window`) can widen the slab.

        `state` = {"x", "v"}: f32[N, 3] by persistent id -- a restart: the scene file says WHAT the particles are, `state`
        where they are and how fast (a slab rank keeps those whose restart position lies in its layers).

        `populate=False` stops where the reference's constructor stands after its allocations
        (particle_system.py:91-145): every field exists with `particle_max_num` zeroed rows and
        `particle_num[None] == 0`; the caller fills it with `add_cube` / `add_particles`, as the
        reference's own constructor does next (:148-211)."""
        self.cfg = config
        self.GGUI = GGUI
        self.slab = slab
        self._restarted = state is not None     # SPHBase.initialize / SlabSolver.initialize: rest cm from x_0, not from x
        x_filter = None
        if slab is not None:
            g0 = _scene.Geometry(config)
            nx = int(g0.grid_num[0])
            x_filter = lambda xs: ((_scene.x_layer_of(xs, g0.grid_size, nx) >= slab["x_lo"])
                                   & (_scene.x_layer_of(xs, g0.grid_size, nx) < slab["x_hi"]))
        sc = _scene.build_scene(config, base_dir=scene_dir, verbose=verbose, x_filter=x_filter, state=state)
        g = sc.geom
        self._scene = sc
        # ---- scalars, same names as the reference (particle_system.py:17-46) ----
        self.domain_start = g.domain_start
        self.domain_end = g.domain_end
        self.domain_size = g.domain_size
        self.dim = g.dim
        self.simulation_method = config.get_cfg("simulationMethod")
        self.material_solid = _scene.MATERIAL_SOLID
        self.material_fluid = _scene.MATERIAL_FLUID
        self.particle_radius = g.particle_radius
        self.particle_diameter = g.particle_diameter
        self.support_radius = g.support_radius
        self.m_V0 = g.m_V0
        self.grid_size = g.grid_size
        self.grid_num = g.grid_num
        self.padding = g.padding
        self.object_collection = sc.object_collection
        self.object_id_rigid_body = sc.object_id_rigid_body
        self.fluid_particle_num = sc.fluid_particle_num
        self.solid_particle_num = sc.solid_particle_num
        self.particle_max_num = sc.particle_max_num
        self.num_rigid_bodies = sc.num_rigid_bodies
        self.particle_num = HostScalar(0, int)
        if verbose:
            print("grid size: ", self.grid_num)
            print(f"Current particle num: {self.particle_num[None]}, Particle max num: {self.particle_max_num}")

        # ---- device context (replaces the ti.field allocations of :91-145) ----
        self._lib = _lib.load()
        self._params = self._make_params(sc)
        slack = int(slab.get("nx_slack", 0)) if slab is not None else 0
        self._params.grid_num[0] += slack            # the allocation; the window is set right below
        ctx = C.c_void_p()
        stream_ptr = C.c_void_p(int(stream)) if stream else None
        rc = self._lib.sph_create(C.byref(self._params), int(device), stream_ptr, C.byref(ctx))
        if rc != 0:
            msg = self._lib.sph_last_error(None)
            raise _lib.SphError(f"sph_create failed (rc={rc}): {msg.decode() if msg else ''}")
        self._ctx = ctx
        if slack:
            self._params.grid_num[0] -= slack
            self._call("sph_slab_set_window", int(self._params.cell_origin[0]), int(self._params.grid_num[0]))
        n = self.count if slab is not None else (lambda: self.particle_max_num)
        F = _lib
        mk = lambda fid, dt, vec=0, w=True, name="": DeviceField(self, fid, dt, n, vec, w, name)
        self.object_id = mk(F.F_OBJECT_ID, np.int32, name="object_id")
        self.x = mk(F.F_X, np.float32, 3, name="x")
        self.x_0 = mk(F.F_X_0, np.float32, 3, name="x_0")
        self.v = mk(F.F_V, np.float32, 3, name="v")
        self.acceleration = mk(F.F_ACCELERATION, np.float32, 3, name="acceleration")
        self.m_V = mk(F.F_M_V, np.float32, name="m_V")
        self.m = mk(F.F_M, np.float32, name="m")
        self.density = mk(F.F_DENSITY, np.float32, name="density")
        self.pressure = mk(F.F_PRESSURE, np.float32, name="pressure")
        self.material = mk(F.F_MATERIAL, np.int32, name="material")
        self.color = mk(F.F_COLOR, np.int32, 3, name="color")
        self.is_dynamic = mk(F.F_IS_DYNAMIC, np.int32, name="is_dynamic")
        self.grid_ids = mk(F.F_GRID_IDS, np.int32, w=False, name="grid_ids")
        self.pid = mk(F.F_PID, np.int32, name="pid")
        if self.simulation_method == 4:                       # particle_system.py:115-117
            self.dfsph_factor = mk(F.F_DFSPH_FACTOR, np.float32, name="dfsph_factor")
            self.density_adv = mk(F.F_DENSITY_ADV, np.float32, name="density_adv")
        self.grid_particles_num = DeviceField(self, F.F_GRID_PARTICLES_NUM, np.int32,
                                              lambda: int(np.prod(self._local_grid_num)), 0, False,
                                              "grid_particles_num")
        if self.num_rigid_bodies > 0:
            self.rigid_rest_cm = DeviceField(self, F.F_RIGID_REST_CM, np.float32, lambda: sc.n_objects, 3, True,
                                             "rigid_rest_cm")
        self._motions = dict(getattr(sc, "motions", {}))     # object id -> motion.Motion; pushed by SPHBase.initialize()
        if self._motions and slab is not None:
            raise NotImplementedError("kinematic bodies (\"motion\" in the scene file) exist on single-domain contexts only")
        self.tracers = None      # the registered tracer set (tracers.Tracers): None until set_tracers
        self.statistics = None   # the registered statistics set (stats.Statistics): None until set_statistics
        self.loads = None        # the registered load set (loads.Loads): None until set_loads
        self.scalars = None      # the registered scalar set (scalars.Scalars): None until set_scalars
        self.features = None     # the registered feature set (features.Features): None until set_features
        self.x_vis_buffer = None
        if self.GGUI:
            self.x_vis_buffer = np.zeros((self.particle_max_num, 3), dtype=np.float32)
            self.color_vis_buffer = np.zeros((self.particle_max_num, 3), dtype=np.float32)

        # ---- upload the initial particles (the reference's _add_particles, :260-284) ----
        if not populate:
            if slab is not None:
                raise ValueError("populate=False is a single-domain feature (a slab rank subsets the scene file)")
            return              # sph_create zero-fills every array (x = 0, material 0 = solid, static), like ti.field
        for name, arr in sc.arrays.items():
            if name == "pid" and slab is None:
                continue            # default pid = index at creation
            getattr(self, name).from_numpy(arr)
        self.particle_num[None] = self.particle_max_num

    # ------------------------------------------------------------------
    def _make_params(self, sc, solver=None):
        g = sc.geom
        cfg = self.cfg
        p = _lib.SphParams()
        if self.slab is None:
            p.n_particles = sc.particle_max_num
            p.capacity = max(sc.particle_max_num, 1)
            local_grid = [int(v) for v in g.grid_num]
            p.cell_origin = (C.c_int32 * 3)(0, 0, 0)
            p.cold_capacity = 0
        else:
            sl = self.slab
            p.n_particles = int(sc.arrays["x"].shape[0])
            p.capacity = max(int(sl["capacity"]), p.n_particles, 1)
            local_grid = [sl["x_hi"] - sl["x_lo"] + 2 * sl["halo"], int(g.grid_num[1]), int(g.grid_num[2])]
            p.cell_origin = (C.c_int32 * 3)(sl["x_lo"] - sl["halo"], 0, 0)
            p.cold_capacity = max(sc.particle_max_num, p.capacity)
        self._local_grid_num = local_grid
        p.grid_num = (C.c_int32 * 3)(*local_grid)
        p.n_objects = sc.n_objects
        p.grid_size = g.grid_size
        p.support_radius = g.support_radius
        p.particle_diameter = g.particle_diameter
        p.m_V0 = g.m_V0
        viscosity = getattr(solver, "viscosity", 0.01)                      # sph_base.py:15
        p.density_0 = getattr(solver, "density_0", cfg.get_cfg("density0") or 1000.0)
        p.stiffness = getattr(solver, "stiffness", cfg.get_cfg("stiffness") or 50000.0)
        p.exponent = getattr(solver, "exponent", cfg.get_cfg("exponent") or 7.0)
        p.viscosity = viscosity
        p.surface_tension = getattr(solver, "surface_tension", 0.01)       # WCSPH.py:15
        p.dt = solver.dt[None] if solver is not None else (cfg.get_cfg("timeStepSize") or 1e-4)
        grav = getattr(solver, "g", None)
        if grav is None:
            grav = cfg.get_cfg("gravitation") or [0.0, -9.81, 0.0]
        p.g = (C.c_float * 3)(*[float(v) for v in grav])
        p.domain_size = (C.c_float * 3)(*[float(v) for v in g.domain_size])
        p.padding = g.padding
        p.wall_hi = (C.c_float * 3)(*[float(v) - g.padding for v in g.domain_size])   # f64 fold, then f32
        kc = _scene.kernel_constants(g.support_radius, viscosity, g.dim)
        p.k_w, p.k_dw, p.visc_d_nu, p.visc_eps = kc["k_w"], kc["k_dw"], kc["visc_d_nu"], kc["visc_eps"]
        return p

    def set_slab_window(self, x_lo, x_hi):
        """Re-cut: this context now owns the global cell layers [x_lo, x_hi) (effective at the next sort)."""
        sl = self.slab
        nx = int(x_hi) - int(x_lo) + 2 * sl["halo"]
        self._call("sph_slab_set_window", int(x_lo) - sl["halo"], nx)   # fails if wider than the allocation (nx_slack)
        sl["x_lo"], sl["x_hi"] = int(x_lo), int(x_hi)
        self._local_grid_num[0] = nx
        self._params.grid_num[0] = nx
        self._params.cell_origin[0] = sl["x_lo"] - sl["halo"]

    def _push_solver_params(self, solver):
        self._params = self._make_params(self._scene, solver)
        self._call("sph_set_params", C.byref(self._params))

    def _call(self, name, *args):
        rc = getattr(self._lib, name)(self._ctx, *args)
        _lib.check(self._lib, self._ctx, rc, name)

    def count(self) -> int:
        """Live particle count of this context (== particle_max_num on a single GPU)."""
        n = C.c_int32()
        self._call("sph_get_particle_count", C.byref(n))
        return int(n.value)

    def set_option(self, option: int, value: int):
        self._call("sph_set_option", int(option), int(value))

    def get_option(self, option: int) -> int:
        v = C.c_int32()
        rc = self._lib.sph_get_option(self._ctx, int(option), C.byref(v))
        _lib.check(self._lib, self._ctx, rc, "sph_get_option")
        return int(v.value)

    def sync(self):
        self._call("sph_sync")

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.sph_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference methods ------------------------------------------------
    def build_solver(self):
        """particle_system.py:214-221."""
        solver_type = self.cfg.get_cfg("simulationMethod")
        if solver_type == 0:
            from .WCSPH import WCSPHSolver
            return WCSPHSolver(self)
        if solver_type == 4:
            from .DFSPH import DFSPHSolver          # (on a slab rank the loops are driven by distributed.SlabSolver)
            return DFSPHSolver(self)
        raise NotImplementedError(f"Solver type {solver_type} has not been implemented.")

    def update_grid_id(self):
        """particle_system.py:311-320."""
        self._call("sph_update_grid_id")

    def prefix_sum(self):
        """self.prefix_sum_executor.run(self.grid_particles_num)  (particle_system.py:374)."""
        self._call("sph_prefix_sum")

    def counting_sort(self):
        """particle_system.py:322-369."""
        self._call("sph_counting_sort")

    def initialize_particle_system(self):
        """particle_system.py:372-375."""
        self.update_grid_id()
        self.prefix_sum()
        self.counting_sort()

    def add_particles(self, object_id, new_particles_num, new_particles_positions, new_particles_velocity,
                      new_particle_density, new_particle_pressure, new_particles_material, new_particles_is_dynamic,
                      new_particles_color):
        """particle_system.py:237-284: rows [particle_num, particle_num + n) of every field take the new particles
        with add_particle's derived values (:222-235: x_0 = x, m_V = m_V0, m = m_V0 * density, acceleration left as
        it is), then particle_num += n.  The fields are fixed-size (`particle_max_num` rows, :101-113): the
        reference writes past their end when more is added than the scene file announced; here that raises.
        Host-side read-modify-write of whole arrays: scene set-up, not a per-step path."""
        n = int(new_particles_num)
        p0 = int(self.particle_num[None])
        if n < 0 or p0 + n > self.particle_max_num:
            raise ValueError(f"add_particles: {p0} + {n} particles exceed particle_max_num = {self.particle_max_num} "
                             "(the fields are sized from the scene file, particle_system.py:52-83)")
        if n == 0:
            return
        if self.slab is not None:
            raise ValueError("add_particles on a slab rank: build the scene before it is cut")
        pos = np.asarray(new_particles_positions, dtype=np.float32).reshape(n, self.dim)
        dens = np.asarray(new_particle_density, dtype=np.float32).reshape(n)
        rows = {
            "object_id": np.full(n, int(object_id), dtype=np.int32),
            "x": pos, "x_0": pos,
            "v": np.asarray(new_particles_velocity, dtype=np.float32).reshape(n, self.dim),
            "density": dens,
            "m_V": np.full(n, self.m_V0, dtype=np.float32),
            "m": (np.float32(self.m_V0) * dens).astype(np.float32),
            "pressure": np.asarray(new_particle_pressure, dtype=np.float32).reshape(n),
            "material": np.asarray(new_particles_material, dtype=np.int32).reshape(n),
            "is_dynamic": np.asarray(new_particles_is_dynamic, dtype=np.int32).reshape(n),
            "color": np.asarray(new_particles_color, dtype=np.int32).reshape(n, 3),
        }
        # (the persistent id of a new row is the id that row already holds: pid is a permutation of the rows at all
        # times -- identity before the first sort -- so x_0 / colour, which are keyed by it, land where the row reads them)
        for name, val in rows.items():
            f = getattr(self, name)
            a = f.to_numpy()
            a[p0:p0 + n] = val
            f.from_numpy(a)
        self.particle_num[None] = p0 + n

    def add_cube(self, object_id, lower_corner, cube_size, material, is_dynamic, color=(0, 0, 0), density=None,
                 pressure=None, velocity=None):
        """particle_system.py:458-495: a lattice of particle_diameter spacing from lower_corner (np.arange per axis,
        'ij' meshgrid, x slowest), constant material / is_dynamic / colour / density (1000 by default) / pressure (0)
        / velocity (0), appended through add_particles."""
        pos = _scene.cube_positions(lower_corner, cube_size, self.particle_diameter, self.dim)
        n = pos.shape[0]
        vel = np.zeros_like(pos) if velocity is None else np.tile(np.asarray(velocity, dtype=np.float32), (n, 1))
        self.add_particles(object_id, n, pos, vel,
                           np.full(n, density if density is not None else 1000.0, dtype=np.float32),
                           np.full(n, pressure if pressure is not None else 0.0, dtype=np.float32),
                           np.full(n, material, dtype=np.int32), np.full(n, is_dynamic, dtype=np.int32),
                           np.tile(np.asarray(color, dtype=np.int32), (n, 1)))
        return n

    def compute_cube_particle_num(self, start, end):
        return _scene.compute_cube_particle_num(start, end, self.particle_diameter, self.dim)

    def dump(self, obj_id):
        """particle_system.py:409-418."""
        mask = (self.object_id.to_numpy() == obj_id).nonzero()
        return {"position": self.x.to_numpy()[mask], "velocity": self.v.to_numpy()[mask]}

    # ---- kinematic bodies (motion.py, include/sph_hip.h; the reference has none) ------
    @property
    def time(self) -> float:
        """Simulated time (f64, held by the context): advanced by dt at the end of every step."""
        t = C.c_double()
        self._call("sph_get_time", C.byref(t))
        return float(t.value)

    @time.setter
    def time(self, value: float):
        self._call("sph_set_time", C.c_double(float(value)))

    def _rest_positions(self, object_id):
        return self.x_0.to_numpy()[self.object_id.to_numpy() == int(object_id)]

    def _push_motions(self):
        """Hand the registered motions to the library (all at once: it replaces the set).  On failure the library keeps
        the set it had."""
        arr = (_lib.SphKinematicMotion * max(len(self._motions), 1))()
        for k, (oid, m) in enumerate(sorted(self._motions.items())):
            arr[k] = _motion.to_struct(oid, m)
        self._call("sph_kinematic_set", arr, len(self._motions))

    def set_body_motion(self, object_id: int, **motion):
        """Prescribe the motion of a non-dynamic solid object from the next step on: the keys of a scene file's
        "motion" entry (linearVelocity, angularVelocity, pivot, oscillation, startTime, endTime; see motion.py).
        Times are on the clock `ps.time`.  Replaces the object's earlier motion."""
        oid = int(object_id)
        obj = self.object_collection.get(oid, {})
        m = _motion.parse_motion(motion, is_dynamic=bool(obj.get("isDynamic")))
        if m.pivot is None:
            rest = self._rest_positions(oid)
            if rest.shape[0] == 0:
                raise ValueError(f"set_body_motion: object {oid} has no particles")
            m.with_pivot(rest)
        if oid not in self._motions and len(self._motions) >= _motion.MAX_KINEMATIC:
            raise ValueError(f"set_body_motion: at most {_motion.MAX_KINEMATIC} objects can be kinematic")
        old = self._motions.get(oid)
        self._motions[oid] = m
        try:
            self._push_motions()
        except _lib.SphError:
            if old is None:
                del self._motions[oid]
            else:
                self._motions[oid] = old
            raise

    def clear_body_motion(self, object_id: int):
        """The object is no longer moved: it stays at the pose of the current time, at rest (a static solid again)."""
        m = self._motions.get(int(object_id))
        if m is None:
            return
        R, c, _, _ = _motion.pose(m, self.time)
        self.set_body_pose(object_id, R, c, pivot=m.pivot)
        del self._motions[int(object_id)]
        self._push_motions()

    def set_body_pose(self, object_id: int, R, origin, lin_vel=(0.0, 0.0, 0.0), ang_vel=(0.0, 0.0, 0.0), pivot=None):
        """Place a non-dynamic solid object now: x = origin + R (x_0 - pivot), v = lin_vel + ang_vel x (x - origin), for
        trajectories scripted from Python.  `pivot` defaults to the mean of the object's rest positions.  Enqueues."""
        p = _lib.SphBodyPose()
        p.object_id = int(object_id)
        if pivot is None:
            rest = self._rest_positions(object_id)
            if rest.shape[0] == 0:
                raise ValueError(f"set_body_pose: object {int(object_id)} has no particles")
            pivot = rest.astype(np.float64).mean(axis=0)
        p.R = (C.c_float * 9)(*[float(v) for v in np.asarray(R, dtype=np.float64).reshape(9)])
        for name, val in (("pivot", pivot), ("origin", origin), ("lin_vel", lin_vel), ("ang_vel", ang_vel)):
            setattr(p, name, (C.c_float * 3)(*[float(v) for v in np.asarray(val, dtype=np.float64).reshape(3)]))
        self._call("sph_kinematic_apply", C.byref(p), 1)

    def _kinematic_reference_step(self, dt: float):
        """What the device loop does at the end of a step, for the step made of individual calls (SPHBase._reference_step):
        the clock advances by the f32 dt the library holds, registered objects go to the pose of the new time."""
        t = self.time + float(np.float32(dt))
        for oid, m in sorted(self._motions.items()):
            R, c, u, w = _motion.pose(m, t)
            self.set_body_pose(oid, R, c, u, w, pivot=m.pivot)
        self.time = t

    def update_kinematic_meshes(self):
        """OBJ export: the export mesh of every kinematic RigidBody at the body's current pose -- R and origin applied to
        `restPosition` on the host, like the dynamic bodies' mesh update (SPHBase.solve_rigid_body)."""
        t = self.time
        for oid, m in self._motions.items():
            obj = self.object_collection.get(oid)
            if obj is not None and "mesh" in obj:
                R, c, _, _ = _motion.pose(m, t)
                obj["mesh"].vertices = c + (np.asarray(obj["restPosition"], dtype=np.float64) - m.pivot) @ R.T

    # ---- flow diagnostics and the CFL-governed time step (diagnostics.py, timestep.py) ------
    def diagnostics(self):
        """Counts, mass, centre of mass, momentum, energies, max |v| / |a|, density / pressure extrema and bounds, per
        object and over all particles, of the state as it is now: one reduction on the device behind whatever was
        enqueued; only the rows are copied back (synchronises).  Changes nothing a later step reads."""
        from . import diagnostics as _diag
        return _diag.reduce(self)

    def column_map(self, axis=1, cell=None, origin=None, shape=None, object_id=None):
        """Depth-integrated map of the fluid over the two axes other than `axis` (columns.ColumnMap): per column the
        particle count, top and bottom of the fluid and the summed velocity; `depth`, `surface`, `velocity`, `gauge(points)`
        and `wet_extent()` follow from them.  `cell` (one number or one per horizontal axis) defaults to the support radius,
        `origin` to 0, `shape` to ceil(domain_size_j / cell); `object_id` restricts the map to one fluid object.  One
        streaming pass on the device behind whatever was enqueued; only the map is copied back (synchronises).  Reads x, v
        and the flags; changes nothing a later step reads."""
        from . import columns as _columns
        return _columns.reduce(self, axis=axis, cell=cell, origin=origin, shape=shape, object_id=object_id)

    def export_particles(self, objects=None, material=None, fields=("velocity",), box=None, every=1, phase=0):
        """The selected particles ORDERED BY PERSISTENT ID, packed on the device into the rows of a binary PLY vertex body
        (export.ParticleExport: `.data` is a structured array x y z [vx vy vz] [density] [pressure] [mass] [id] [object],
        `.write_ply(path)` writes it).  `objects`: ids to keep (None: all); `material`: "fluid", "solid" or an id (None: any);
        `fields`: names from velocity, density, pressure, mass, id, object (the position is always there); `box` = (lo, hi):
        keep lo <= x <= hi; `every`, `phase`: keep pid % every == phase, the same particles in every call.  Row k is the
        same particle in every export of one selection.  One pass on the device behind whatever was enqueued; only the rows
        are copied back (synchronises).  Reads the records; changes nothing a later step reads."""
        from . import export as _export
        return _export.export(self, objects=objects, material=material, fields=fields, box=box, every=every, phase=phase)

    def sample_grid(self, spacing=None, origin=None, shape=None, fields=("velocity",), material="fluid", objects=None, gradients=()):
        """The SPH interpolation of `fields` (names from velocity, density, pressure) at the nodes origin + k * spacing of a
        regular grid (sample.FieldGrid: raw i64 planes `weight`, `count`, `sums`; `fill`, `velocity`, `density`, `pressure`,
        `wet()` follow from them; `write_vtk(path)`).  `spacing` (one number or one per axis) defaults to the particle
        diameter, `origin` to 0, `shape` to the nodes that cover the domain; a slice is a shape with a 1 in it.  `material`:
        "fluid" (default), "solid", an id or None (any; solids then contribute with their boundary volumes); `objects`: ids to
        keep (None: all).  x and v are the current values; density and pressure are those of the last step's density sweep,
        one dt behind.  One streaming pass on the device behind whatever was enqueued; only the planes are copied back
        (synchronises).  Reads the records; changes nothing a later step reads.
        `gradients`: names from `fields` whose analytic gradient the same pass sums as well, or ("fill",) for the fill gradient
        alone, which comes with any of them (raw `grad_fill`, `grad_sums`; `fill_gradient`, `surface_normal`,
        `velocity_gradient`, `vorticity`, `divergence`, `strain_rate`, `q_criterion`, `pressure_gradient`, `density_gradient`).
        () is the call as it was."""
        from . import sample as _sample
        return _sample.sample_grid(self, spacing=spacing, origin=origin, shape=shape, fields=fields, material=material, objects=objects,
                                   gradients=gradients)

    def sample_points(self, points, fields=("velocity",), material="fluid", objects=None, gradients=()):
        """The same interpolation at up to 1024 probe points [[x, y, z], ...] (sample.FieldProbes: the same planes and views per
        point, `rows()` for JSON); `gradients` as for `sample_grid`."""
        from . import sample as _sample
        return _sample.sample_points(self, points, fields=fields, material=material, objects=objects, gradients=gradients)

    def surface_mesh(self, spacing=None, origin=None, shape=None, iso=0.4, cap=True, material="fluid", objects=None):
        """The surface of the selected particles as an indexed triangle mesh (mesh.SurfaceMesh: `vertices`, `normals`,
        `triangles`; `volume()`, `area()`, `is_closed()`, `write_ply(path)`): surface nets on the grid `sample_grid` would make
        from the same `spacing`, `origin`, `shape` (every node count at least 2), `material` and `objects`.  The surface is
        where the grid's fill (weight / 2^30) equals `iso`; the fill is about 0.8 inside a fluid at rest spacing, so the default
        0.4 is half the interior fill.  `cap`: treat the grid's outer layer of nodes as empty, which closes the mesh where the
        fluid meets the grid's border (without it the mesh is open there).  With material=None the solids join the surface.
        The grid is sampled and the mesh built on the device behind whatever was enqueued; only the mesh is copied back
        (synchronises).  Reads the records; changes nothing a later step reads."""
        from . import mesh as _mesh
        return _mesh.surface_mesh(self, spacing=spacing, origin=origin, shape=shape, iso=iso, cap=cap, material=material, objects=objects)

    def set_tracers(self, points, min_fill=0.2, record_every=0, record_capacity=0, material="fluid", objects=None):
        """Register passive tracers at `points` [[x, y, z], ...] (up to 2^22, inside [padding, domain_size - padding]): from now on
        every step of the device loop (`solver.step(n)`) moves each of them with the Shepard mean of the velocity of the selected
        particles (`material`, `objects` as for `sample_grid`) in the 27 cells around it, on the device.  A tracer whose Shepard
        sum is below `min_fill` stays where it is for that step (0.2 is a quarter of the 0.8 inside fluid at rest spacing: below
        it the mean rests on one or two particles).  `record_every=k` with `record_capacity=n` keeps the positions after every
        k-th advance, up to n frames, on the device (`tracers.paths()`).  Replaces the set; returns `self.tracers`
        (tracers.Tracers).  Tracers are not part of `save_state`."""
        from . import tracers as _tracers
        self.tracers = _tracers.set_tracers(self, points, min_fill=min_fill, record_every=record_every,
                                            record_capacity=record_capacity, material=material, objects=objects)
        return self.tracers

    def clear_tracers(self):
        """Remove the tracer set: the steps enqueue what they did before any was set.  `self.tracers` becomes an empty set."""
        from . import tracers as _tracers
        self.tracers = _tracers.clear_tracers(self)

    def set_statistics(self, origin=None, spacing=None, shape=None, objects=None, material="fluid", every=10, capacity=None, wet=0.4):
        """Register running flow statistics on a grid (`origin`, `spacing`, `shape`, `objects`, `material` exactly as for
        `sample_grid`; a slice is a shape with a 1 in it): from now on every `every`-th step of the device loop (`solver.step(n)`)
        samples the Shepard-mean velocity of the selected particles at the nodes and folds it into integer accumulators on the
        device; a node counts as wet in a sample when its Shepard sum reaches `wet`.  `capacity` bounds the number of samples
        (default and maximum 2^19).  A whole-domain volume costs many steps' worth of time per sample -- `every` is what makes it
        affordable -- while a slice can run every step ("Running flow statistics").  Replaces the set; returns
        `self.statistics` (stats.Statistics): mean_velocity(), reynolds_stress(), rms_velocity(), tke(), intermittency(),
        mean_fill(), accumulators(), write_vtk(path), reset().  Statistics are not part of `save_state`."""
        from . import stats as _stats
        self.statistics = _stats.set_statistics(self, spacing=spacing, origin=origin, shape=shape, objects=objects, material=material,
                                                every=every, capacity=capacity, wet=wet)
        return self.statistics

    def clear_statistics(self):
        """Remove the statistics set: the steps enqueue what they did before any was set.  `self.statistics` becomes None."""
        from . import stats as _stats
        _stats.clear_statistics(self)
        self.statistics = None

    def set_loads(self, objects=(1,), about=(0.0, 0.0, 0.0), every=1, capacity=4096):
        """Register fluid loads on the solid `objects` (1 to 32 ids; static, kinematic or dynamic): from now on every `every`-th
        WCSPH step of the device loop (`solver.step(n)`) samples, behind the step's density and pressure and before its force sweep,
        the force and the torque about the world point `about` that the fluid exerts on each object -- the Akinci boundary term
        of the force sweep, summed in integers on the device, so the series is one function of the run.  `capacity` bounds the
        samples kept.  Replaces the set; returns `self.loads` (loads.Loads): force(), torque(about=None), pairs(), wet_particles(),
        saturated(), times, impulse(), rows(), write_csv(path), sample(), reset().  A DFSPH step refuses to run with a set
        registered.  Loads are not part of `save_state`."""
        from . import loads as _loads
        self.loads = _loads.set_loads(self, objects=objects, about=about, every=every, capacity=capacity)
        return self.loads

    def clear_loads(self):
        """Remove the load set: the steps enqueue what they did before any was set.  `self.loads` becomes None."""
        from . import loads as _loads
        _loads.clear_loads(self)
        self.loads = None

    def set_scalars(self, channels=("dye",), diffusivity=(1e-4,), values=None, sources=None, every=1, material="fluid", objects=None):
        """Register carried scalars: 1 to 4 named `channels` that ride on the selected particles (`material`, `objects`: the
        carriers) and diffuse between neighbouring carriers with `diffusivity` (m^2/s per channel) on the device, every `every`-th
        step of the device loop (`solver.step(n)`, WCSPH or DFSPH) right behind its sort, with a = dt * every * diffusivity.
        `values`: None (zeros), an array [n_ids, K] by persistent id, or {object id: row}; `sources`: {object id: row} of up to 8
        objects (fluid or solid) that hold a prescribed value; every other particle is invisible to the sum (insulation).
        Replaces the set; returns `self.scalars` (scalars.Scalars): values(), raw(), total(channel), range(channel), overshoot(),
        saturated(), samples, paint(channel, range=None, colormap="heat"), save(path), sample().  Positions and velocities of
        a run with a set are bit-identical to the run without.  Scalars are not part of `save_state`."""
        from . import scalars as _scalars
        self.scalars = _scalars.set_scalars(self, channels=channels, diffusivity=diffusivity, values=values, sources=sources, every=every,
                                            material=material, objects=objects)
        return self.scalars

    def clear_scalars(self):
        """Remove the scalar set: the steps enqueue what they did before any was set.  `self.scalars` becomes None."""
        from . import scalars as _scalars
        _scalars.clear_scalars(self)
        self.scalars = None

    def set_features(self, every=10, material="fluid", objects=None, min_neighbours=24, normal_min=0.0):
        """Register per-particle flow features of the selected particles (`material`, `objects`: the selection of the other
        observers): from now on every `every`-th WCSPH step samples, behind its density and before its force sweep, vorticity,
        divergence, colour gradient, kernel fill, neighbour counts and a free-surface flag (fewer than `min_neighbours` neighbours, or
        h |N| above `normal_min` when that is positive) of each of them on the device, one row per persistent id, the latest sample
        only.  A sample walks the 27 cells of every selected particle -- several steps' time -- so `every` > 1 is the normal use.
        Replaces the set; returns `self.features` (features.Features): vorticity(), divergence(), fill(), neighbours(), normal(),
        surface(), valid(), saturated(), positions(), ids, time, step, samples, enstrophy(), sample(), write_ply(), paint()."""
        from . import features as _features
        self.features = _features.set_features(self, every=every, material=material, objects=objects, min_neighbours=min_neighbours,
                                               normal_min=normal_min)
        return self.features

    def clear_features(self):
        """Remove the feature set: the steps enqueue what they did before any was set.  `self.features` becomes None."""
        from . import features as _features
        _features.clear_features(self)
        self.features = None

    def _step_call(self, name, n_steps, ids, n_ids, dt):
        """sph_step / sph_dfsph_step; with tracers registered, the times of the history frames the call stored are noted."""
        tr = self.tracers if self.tracers is not None and self.tracers.m > 0 else None
        t0 = self.time if tr is not None else 0.0
        try:
            self._call(name, int(n_steps), ids, n_ids)
        finally:
            if tr is not None:
                tr._after_steps(t0, dt)

    def build_time_step_controller(self, solver):
        """A `timestep.TimeStepController` if the scene's Configuration has an "adaptiveTimeStep" object, else None."""
        from . import timestep as _timestep
        return _timestep.build_controller(self, solver)

    # ---- state checkpoint (the reference has none) ----------------------
    _STATE_FIELDS = ("object_id", "x", "x_0", "v", "acceleration", "m_V", "m", "density", "pressure", "material",
                     "color", "is_dynamic", "pid")

    def save_state(self, path: str, **meta):
        """Every per-particle array in the current (cell-sorted) order + rigid_rest_cm, as one .npz.  Restoring it
        into a ParticleSystem built from the same scene continues the run exactly where it stopped."""
        data = {}
        for f in self._STATE_FIELDS:
            try:
                data[f] = getattr(self, f).to_numpy()
            except _lib.SphError:
                # a slab rank right after a fused sph_slab_forces: the interior accelerations were consumed in the sweep's
                # finish and never written out (sph_download refuses stale values).  The field is dead across steps --
                # every step rewrites it before reading it -- so the checkpoint carries zeros.
                if f != "acceleration":
                    raise
                data[f] = np.zeros((self.count() if self.slab is not None else self.particle_max_num, 3), dtype=np.float32)
        if self.num_rigid_bodies > 0:
            data["rigid_rest_cm"] = self.rigid_rest_cm.to_numpy()
        data["particle_max_num"] = np.int64(self.particle_max_num)
        data["sim_time"] = np.float64(self.time)       # the clock: a restarted run continues a prescribed motion exactly
        for k, v in meta.items():
            data["meta_" + k] = np.asarray(v)
        np.savez_compressed(path, **data)

    def load_state(self, path: str):
        z = np.load(path)
        if int(z["particle_max_num"]) != self.particle_max_num:
            raise ValueError(f"checkpoint holds {int(z['particle_max_num'])} particles, this scene {self.particle_max_num}")
        self.pid.from_numpy(z["pid"])                  # first: x_0 / color are keyed by the persistent id
        for f in self._STATE_FIELDS:
            if f != "pid":
                getattr(self, f).from_numpy(z[f])
        if "rigid_rest_cm" in z.files and self.num_rigid_bodies > 0:
            self.rigid_rest_cm.from_numpy(z["rigid_rest_cm"])
        if "sim_time" in z.files:
            self.time = float(z["sim_time"])
        return {k[5:]: z[k] for k in z.files if k.startswith("meta_")}

    # ---- frame export (run_simulation.py:37-98 of the reference: the window; here an image made on the device) ----
    def _set_view(self, camera, invisible_objects, size):
        """Camera parameters and invisible list of the next frame, of either style; returns the image's (H, W)."""
        from . import render as _render
        cam = camera if camera is not None else _render.Camera()
        rp = _render.render_params(cam, size, self.particle_radius, self.domain_end)
        self._call("sph_render_set_params", C.byref(rp))
        ids = [int(i) for i in invisible_objects]
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        self._call("sph_render_set_invisible", arr, len(ids))
        return (int(size[1]), int(size[0]))

    def _frame_plane(self, shape_attr, symbol, missing):
        """float32 [H, W] plane `symbol` downloads of the last frame whose shape `shape_attr` holds."""
        shape = getattr(self, shape_attr, None)
        if shape is None:
            raise _lib.SphError(missing)
        out = np.empty(shape, dtype=np.float32)
        self._call(symbol, out.ctypes.data_as(C.c_void_p), out.nbytes)
        return out

    def field_range(self, field, material="fluid", objects=None, invisible_objects=()):
        """(lo, hi, count, non_finite) of `field` (render.FIELDS; a position is taken as it is) over the particles that `material`
        and `objects` select as a `render.FieldColour` does and that are not of an invisible object: minimum and maximum of the
        finite values, their number, and the number of values that are not finite.  Over no particle: (inf, -inf, 0, n).  One
        streaming pass on the device behind whatever was enqueued; 24 bytes are copied back (synchronises).  Exact for any
        particle order."""
        from . import render as _render
        return self._field_range(_render.FieldColour(field, material=material, objects=objects), invisible_objects)

    def _field_range(self, colour, invisible_objects):
        from . import render as _render
        ids = [int(i) for i in invisible_objects]
        self._call("sph_render_set_invisible", (C.c_int32 * max(len(ids), 1))(*ids), len(ids))
        fp, out = _render.field_colour_params(colour), _lib.SphFieldRange()
        self._call("sph_field_range", C.byref(fp), C.byref(out))
        return float(out.lo), float(out.hi), int(out.count), int(out.non_finite)

    def _set_colour(self, colour, invisible_objects):
        """The colouring of the next frame, of either style: None switches it off (a context that never had one is not
        touched); else the range is the colouring's or, reduced on the device, that of the particles it colours.  The range in
        force is kept in `frame_colour_range`."""
        from . import render as _render
        if colour is None:
            if getattr(self, "_colour_on", False):
                self._call("sph_frame_set_colour", None, None)
                self._colour_on = False
            self.frame_colour_range = None
            return
        if not isinstance(colour, _render.FieldColour):
            raise TypeError("colour must be a render.FieldColour or None")
        rng = colour.range
        if rng is None:
            lo, hi, count, _ = ParticleSystem._field_range(self, colour, invisible_objects)
            rng = _render.auto_range(lo, hi, count)
        fp = _render.field_colour_params(colour, rng)
        lut = colour.lut()
        self._call("sph_frame_set_colour", C.byref(fp), lut.ctypes.data_as(C.c_void_p))
        self._colour_on = True
        self.frame_colour_range = (float(np.float32(rng[0])), float(np.float32(rng[1])))

    def render(self, camera=None, invisible_objects=(), size=(1024, 1024), colour=None) -> np.ndarray:
        """The particles as lit spheres of radius `particle_radius` in their objects' colours plus the domain box, seen
        from `camera` (default: the reference's window camera), as uint8 [H, W, 3] with row 0 at the top; `size` =
        (width, height).  `colour`: a `render.FieldColour` -- the particles it selects are coloured by a field (speed, density,
        pressure, height ...) through a colour table instead; None: every particle in its object's colour.  Rendered on the GPU
        behind whatever was enqueued before; only the image is copied back.  Independent of `GGUI` and of `copy_to_vis_buffer`."""
        shape = ParticleSystem._set_view(self, camera, invisible_objects, size)   # (by class: stand-ins borrow this method alone)
        ParticleSystem._set_colour(self, colour, invisible_objects)
        self._call("sph_render_frame")
        self._render_shape = shape
        out = np.empty(shape + (3,), dtype=np.uint8)
        self._call("sph_render_download", out.ctypes.data_as(C.c_void_p), out.nbytes)
        return out

    def render_depth(self) -> np.ndarray:
        """float32 [H, W] of the last `render`: distance along the view direction of the surface (or box line) each
        pixel shows, +inf where nothing was drawn."""
        return self._frame_plane("_render_shape", "sph_render_download_depth", "render_depth: no frame has been rendered")

    # ---- surface frames (csrc/sph_surface.hip; the reference's window has no such style) ----
    def _first_fluid_colour(self):
        blocks = self.cfg.get_fluid_blocks()
        return tuple(blocks[0].get("color", (50, 100, 200))) if blocks else (50, 100, 200)

    def render_surface(self, camera=None, invisible_objects=(), size=(1024, 1024), style=None, colour=None) -> np.ndarray:
        """The fluid as ONE shaded surface -- screen-space depth and thickness, the depth smoothed in image space, normals
        from it, absorption by thickness, Fresnel and a highlight -- over the solids and the domain box drawn as `render`
        draws them; uint8 [H, W, 3] with row 0 at the top.  `style`: a `render.SurfaceStyle` (None: its defaults, with the
        filter radius 3 x and the depth range 4 x the particle radius and the first fluid block's colour).  `colour`: a
        `render.FieldColour` -- the surface's body colour comes from the field at the visible surface (the table index of each
        pixel's nearest selected fluid particle, smoothed like the thickness), selected solids are coloured as `render` colours
        them; None: the style's fluid colour.  Rendered on the GPU behind whatever was enqueued before; only the image is copied
        back.  Reads the particles; changes nothing."""
        from . import render as _render
        shape = ParticleSystem._set_view(self, camera, invisible_objects, size)   # (by class: stand-ins borrow this method alone)
        ParticleSystem._set_colour(self, colour, invisible_objects)
        sp =_render.surface_params(_render.resolve_style(style, self.particle_radius, self._first_fluid_colour()))
        self._call("sph_surface_set_params", C.byref(sp))
        self._call("sph_surface_frame")
        self._surface_shape = shape
        out = np.empty(shape + (3,), dtype=np.uint8)
        self._call("sph_surface_download", out.ctypes.data_as(C.c_void_p), out.nbytes)
        return out

    def _surface_plane(self, symbol, what):
        return self._frame_plane("_surface_shape", symbol, f"{what}: no surface frame has been rendered")

    def render_surface_depth(self) -> np.ndarray:
        """float32 [H, W] of the last `render_surface`: the smoothed fluid depth where the fluid is shown, else the depth of
        the solid or box line behind, +inf where nothing was drawn."""
        return self._surface_plane("sph_surface_download_depth", "render_surface_depth")

    def render_surface_thickness(self) -> np.ndarray:
        """float32 [H, W] of the last `render_surface`: the smoothed thickness of the fluid in front of the solids along
        each pixel's ray, in world units; 0 where no fluid is shown."""
        return self._surface_plane("sph_surface_download_thickness", "render_surface_thickness")

    def render_surface_field_index(self) -> np.ndarray:
        """int32 [H, W] of the last `render_surface` made with a `colour` that selects fluid: the smoothed colour-table index
        of each pixel's fluid, -1 where the pixel holds no field-coloured fluid."""
        shape = getattr(self, "_surface_shape", None)
        if shape is None:
            raise _lib.SphError("render_surface_field_index: no surface frame has been rendered")
        out = np.empty(shape, dtype=np.int32)
        self._call("sph_frame_download_field_index", out.ctypes.data_as(C.c_void_p), out.nbytes)
        return out

    def copy_to_vis_buffer(self, invisible_objects=[]):
        """particle_system.py:392-407 (host copy; there is no GGUI here)."""
        assert self.GGUI
        oid = self.object_id.to_numpy()
        x = self.x.to_numpy()
        col = self.color.to_numpy()
        if len(invisible_objects) != 0:
            self.x_vis_buffer[:] = 0.0
            self.color_vis_buffer[:] = 0.0
        vis = ~np.isin(oid, list(invisible_objects)) & np.isin(oid, list(self.object_collection.keys()))
        self.x_vis_buffer[vis] = x[vis]
        self.color_vis_buffer[vis] = col[vis] / 255.0
