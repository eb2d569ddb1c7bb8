"""A numpy model of the running flow statistics (include/sph_hip.h, section "Running flow statistics"): one sample is the scatter
sums of tests/sample_model.py (fields vx vy vz) followed by the fold, written exactly as the contract states it -- astype(np.float64)
for the i64 -> f64 conversion, `/` for the divide, np.clip for the clamp, np.rint(...).astype(np.int64) for the rounding -- and the
accumulation is integer addition.  It knows nothing of lanes, pairs of nodes or 16-byte accesses.
"""
import numpy as np

from tests import sample_model

U_LIMIT = 1024.0
U_SCALE, UU_SCALE = 2.0 ** 32, 2.0 ** 24
UU_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
KEYS = ("n_wet", "sum_w", "sum_u", "sum_uu")


def fresh(nodes):
    """Zeroed accumulators over `nodes` nodes."""
    return {"n_wet": np.zeros(nodes, np.int64), "sum_w": np.zeros(nodes, np.int64), "sum_u": np.zeros((3, nodes), np.int64),
            "sum_uu": np.zeros((6, nodes), np.int64), "samples": 0}


def wet_min(wet):
    return int(np.rint(np.float64(wet) * 2 ** 30))


def fold(acc, weight, sums, wet_min_):
    """A new accumulator dict: `acc` with one sample folded in.  weight i64 [nodes], sums i64 [3, nodes] (S_x, S_y, S_z)."""
    weight = np.asarray(weight, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.int64).reshape(3, -1)
    wet = (weight >= int(wet_min_)) & (weight > 0)
    out = {k: acc[k].copy() for k in KEYS}
    out["samples"] = acc["samples"] + 1
    W = np.where(wet, weight, 1).astype(np.float64)                  # (no division is evaluated for a node that is not wet)
    u = [np.clip(sums[a].astype(np.float64) / W, -U_LIMIT, U_LIMIT) for a in range(3)]
    out["n_wet"] += wet.astype(np.int64)
    out["sum_w"] += np.where(wet, weight, 0)
    for a in range(3):
        out["sum_u"][a] += np.where(wet, np.rint(u[a] * U_SCALE).astype(np.int64), 0)
    for k, (a, b) in enumerate(UU_PAIRS):
        out["sum_uu"][k] += np.where(wet, np.rint((u[a] * u[b]) * UU_SCALE).astype(np.int64), 0)
    return out


def fold_velocity(acc, u, weight, wet_min_=1):
    """One sample whose every node sees the velocity u (f64 [3] or [nodes, 3]) with the Shepard weight `weight` (i64): the scatter
    sums a single particle of that weight would leave (S_a = rint(weight * u_a)), folded."""
    weight = np.broadcast_to(np.asarray(weight, dtype=np.int64), acc["n_wet"].shape)
    u = np.broadcast_to(np.asarray(u, dtype=np.float64), acc["n_wet"].shape + (3,))
    sums = np.rint(weight.astype(np.float64)[None, :] * u.T).astype(np.int64)
    return fold(acc, weight, sums, wet_min_)


def sample(acc, positions, x, v, m_V, selected, inv_h, k_w, wet_min_):
    """One sample of the particle state at the node `positions` (f32 [nodes, 3]) folded into `acc`."""
    s = sample_model.sample(positions, x, m_V, [v[:, 0], v[:, 1], v[:, 2]], selected, inv_h, k_w)
    return fold(acc, s["weight"], s["sums"], wet_min_)
