"""The observers agree on who is selected: for one table of selections the export's `selected`, the field range's count and the
sampler's `count` at a probe equal the numbers counted on the host from the downloaded `material` and `object_id` arrays.  Every
quantity is an integer count, so every comparison is exact."""
import numpy as np
import pytest

from sph_taichi_amd import export
from tests import sample_model as model
from tests import scenes

pytestmark = pytest.mark.gpu

FLUID, SOLID = 1, 0
UNUSED = list(range(1000, 1032))                      # 32 ids no object of the scene has
# name -> (material, objects); the scene's objects: 0 the fluid, 1 the static slab, 2 the dynamic cube
SELECTIONS = {
    "all": (None, None),
    "fluid": ("fluid", None),
    "solid": ("solid", None),
    "one object": (None, [0]),
    "last of 32 slots": (None, UNUSED[:31] + [2]),    # the id loop's last trip
    "32 ids, none present": (None, UNUSED),
    "fluid material, a solid's id": ("fluid", [1]),
}
SAMPLED = ("one object", "last of 32 slots")


@pytest.fixture(scope="module")
def state():
    ps, solver = scenes.make_ps(scenes.fluid_with_rigid_blocks())
    solver.initialize()
    solver.step(1)
    f = {name: getattr(ps, name).to_numpy() for name in ("x", "m_V", "material", "object_id")}
    yield ps, f
    ps.close()


def _host(f, material, objects):
    return model.select(f["material"], f["object_id"], -1 if material is None else {"fluid": FLUID, "solid": SOLID}[material], objects or ())


def test_the_scene_has_what_the_table_needs(state):
    _, f = state
    assert sorted(set(f["object_id"].tolist())) == [0, 1, 2] and sorted(set(f["material"].tolist())) == [SOLID, FLUID]
    assert set(f["material"][f["object_id"] == 0].tolist()) == {FLUID} and set(f["material"][f["object_id"] != 0].tolist()) == {SOLID}
    assert f["x"].shape[0] > 256                      # more than one block of every walk
    counts = {name: int(_host(f, *sel).sum()) for name, sel in SELECTIONS.items()}
    n = {k: int((f["object_id"] == k).sum()) for k in (0, 1, 2)}
    assert counts == {"all": n[0] + n[1] + n[2], "fluid": n[0], "solid": n[1] + n[2], "one object": n[0], "last of 32 slots": n[2],
                      "32 ids, none present": 0, "fluid material, a solid's id": 0}


@pytest.mark.parametrize("name", list(SELECTIONS))
def test_export_and_field_range_count_the_host_s_particles(state, name):
    ps, f = state
    material, objects = SELECTIONS[name]
    want = int(_host(f, material, objects).sum())
    info = export.select_info(ps, export.make_params(export.select_args(objects=objects, material=material, fields=())))
    rng = ps.field_range("speed", material=material, objects=objects)
    print(f"{name}: host {want}, export selected {info.selected}, field range {rng[2]} + {rng[3]}")
    assert info.selected == want and info.duplicate_ids == 0
    assert rng[2] + rng[3] == want
    assert info.selected == rng[2] + rng[3]


def test_the_sampler_counts_the_host_s_particles_at_a_probe(state):
    ps, f = state
    # the fluid particle closest to the cube: selected particles of both sampled selections lie inside its support radius
    fluid, cube = np.flatnonzero(f["object_id"] == 0), np.flatnonzero(f["object_id"] == 2)
    d2 = ((f["x"][fluid][:, None, :].astype(np.float64) - f["x"][cube][None, :, :].astype(np.float64)) ** 2).sum(axis=2)
    probe = f["x"][fluid[np.unravel_index(np.argmin(d2), d2.shape)[0]]]
    inside, _ = model.pair_weight(probe[None, None, :], f["x"][None, :, :], f["m_V"][None, :], model.inv_h(ps.support_radius), model.k_w(ps.support_radius))
    for name in SAMPLED:
        material, objects = SELECTIONS[name]
        want = int((inside[0] & _host(f, material, objects)).sum())
        got = ps.sample_points([probe], fields=(), material=material, objects=objects)
        print(f"{name}: host {want} within the support radius of {probe.tolist()}, sampler count {int(got.count[0])}")
        assert want > 0
        assert int(got.count[0]) == want
