"""A numpy restatement of the posed-geometry formulas (audio2photoreal_amd/skinning.py, the reference's visualize/ca_body/utils/
lbs.py and quaternion.py), written from the mathematics.  Test infrastructure: the yardstick of tests/test_skinning_hip.py and
tests/test_skinning_cpu.py, and what tests/golden/make_golden_skinning.py measures the reference's own float32 error against.

Every function takes `dtype` (float64 by default): all inputs are cast to it and every operation runs in it.  The float32 run
against the float64 run is the rounding error float32 arithmetic makes on a skeleton: the allowance of the GPU tests for
skeletons that are not in the fixture.

A skeleton is a dict of arrays: parents [J] (negative = root), pre_rotation [J, 4] (xyzw), joint_offset [J, 3], transform
[7 J, P], transform_offsets [7 J], skin_indices / skin_weights [V, K], rest_vertices [V, 3]."""
import numpy as np


def qmul(q, r):
    """Hamilton product of xyzw quaternions [..., 4]."""
    qx, qy, qz, qw = (q[..., i] for i in range(4))
    rx, ry, rz, rw = (r[..., i] for i in range(4))
    return np.stack([qw * rx + qx * rw + qy * rz - qz * ry,
                     qw * ry - qx * rz + qy * rw + qz * rx,
                     qw * rz + qx * ry - qy * rx + qz * rw,
                     qw * rw - qx * rx - qy * ry - qz * rz], axis=-1)


def qrot(q, v):
    """Rotate v [..., 3] by the (not necessarily unit) quaternion q the way the reference does: v + 2 (w a x v + a x (a x v))."""
    a = q[..., :3]
    av = np.cross(a, v)
    aav = np.cross(a, av)
    return v + 2 * (av * q[..., 3:4] + aav)


def qinv(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0], q.dtype) / (q * q).sum(axis=-1, keepdims=True)


def from_xyz(r):
    """XYZ Euler angles [..., 3] -> xyzw quaternion; half angles (-0.5, 0.5, 0.5) as in Quaternion.batchFromXYZ."""
    h = r * np.array([-0.5, 0.5, 0.5], r.dtype)
    c, s = np.cos(h), np.sin(h)
    c0, c1, c2 = c[..., 0], c[..., 1], c[..., 2]
    s0, s1, s2 = s[..., 0], s[..., 1], s[..., 2]
    return np.stack([-s0 * c1 * c2 - c0 * s1 * s2,
                     c0 * s1 * c2 - s0 * c1 * s2,
                     c0 * c1 * s2 + s0 * s1 * c2,
                     c0 * c1 * c2 - s0 * s1 * s2], axis=-1)


def joint_parameters(skel, poses, scales, dtype=np.float64):
    """[N, 7 J] = cat(poses, scales) @ transform^T + offsets; scales [1, .] is shared by every frame."""
    poses, scales = np.asarray(poses, dtype), np.asarray(scales, dtype)
    scales = np.broadcast_to(scales.reshape(-1, scales.shape[-1]), (poses.shape[0], scales.shape[-1]))
    x = np.concatenate([poses, scales], axis=1)
    return x @ np.asarray(skel["transform"], dtype).T + np.asarray(skel["transform_offsets"], dtype).reshape(1, -1)


def solve_states(skel, params, dtype=np.float64):
    """[N, 7 J] joint parameters -> [N, J, 8] global states (translation, quaternion xyzw, scale)."""
    params = np.asarray(params, dtype)
    N = params.shape[0]
    jp = params.reshape(N, -1, 7)
    J = jp.shape[1]
    parents = np.asarray(skel["parents"]).reshape(-1)
    lt = jp[:, :, 0:3] + np.asarray(skel["joint_offset"], dtype)[None]
    lr = qmul(np.asarray(skel["pre_rotation"], dtype)[None], from_xyz(jp[:, :, 3:6]))
    ls = np.exp2(jp[:, :, 6])
    out = np.zeros((N, J, 8), dtype)
    for j in range(J):
        p = int(parents[j])
        if p < 0 or p >= J:
            out[:, j, 0:3], out[:, j, 3:7], out[:, j, 7] = lt[:, j], lr[:, j], ls[:, j]
        else:
            assert p < j, "a parent must precede its child"
            pq, ps = out[:, p, 3:7], out[:, p, 7:8]
            out[:, j, 3:7] = qmul(pq, lr[:, j])
            out[:, j, 0:3] = qrot(pq, lt[:, j] * ps) + out[:, p, 0:3]
            out[:, j, 7] = ps[:, 0] * ls[:, j]
    return out


def joint_states(skel, poses, scales, dtype=np.float64):
    return solve_states(skel, joint_parameters(skel, poses, scales, dtype), dtype)


def bind_state(skel, dtype=np.float64):
    """[1, J, 8]: the states of the all-zero parameter vector."""
    offs = np.asarray(skel["transform_offsets"], dtype).reshape(1, -1)
    return solve_states(skel, offs, dtype)


def states_to_matrix(bind, states, dtype=np.float64):
    """[N, J, 3, 4] = state o bind^-1 as [R s | t] (row, column): the reference's states_to_matrix."""
    bind, states = np.asarray(bind, dtype), np.asarray(states, dtype)
    br = qinv(bind[:, :, 3:7])
    bs = 1 / bind[:, :, 7:8]
    bt = qrot(br, -bind[:, :, 0:3]) * bs
    tr = qmul(states[:, :, 3:7], np.broadcast_to(br, states[:, :, 3:7].shape))
    ts = states[:, :, 7:8] * bs
    tt = qrot(states[:, :, 3:7], bt * states[:, :, 7:8]) + states[:, :, 0:3]
    x, y, z, w = (tr[..., i] for i in range(4))
    rot = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=-1),
                    np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=-1),
                    np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1)], axis=-2)
    return np.concatenate([rot * ts[..., None], tt[..., None]], axis=-1)


def transforms(skel, poses, scales, dtype=np.float64):
    return states_to_matrix(bind_state(skel, dtype), joint_states(skel, poses, scales, dtype), dtype)


def skin(skel, mats, verts, dtype=np.float64):
    """[N, V, 3] = sum_k w[v, k] (mats[n, idx[v, k]] [verts[n or 0, v], 1])."""
    mats, verts = np.asarray(mats, dtype), np.asarray(verts, dtype)
    verts = verts.reshape((-1,) + verts.shape[-2:])
    idx = np.asarray(skel["skin_indices"])
    w = np.asarray(skel["skin_weights"], dtype)
    out = np.zeros((mats.shape[0], idx.shape[0], 3), dtype)
    for k in range(idx.shape[1]):
        m = mats[:, idx[:, k]]                                                 # [N, V, 3, 4]
        p = np.einsum("nvrc,nvc->nvr", m[..., :3], np.broadcast_to(verts, out.shape)) + m[..., 3]
        out += p * w[None, :, k, None]
    return out


def pose_vertices(skel, poses, scales, verts_unposed=None, template_verts=None, global_scaling=1.0, dtype=np.float64):
    """LBSModule.pose: skin (verts_unposed + template) and multiply by global_scaling; without verts_unposed, skin the template
    (the rest vertices when there is none)."""
    base = np.asarray(skel["rest_vertices"] if template_verts is None else template_verts, dtype)
    verts = base if verts_unposed is None else np.asarray(verts_unposed, dtype) + base
    out = skin(skel, transforms(skel, poses, scales, dtype), verts, dtype)
    return out * np.asarray(global_scaling, dtype)


def joint_positions(skel, poses, scales, global_scaling=1.0, dtype=np.float64):
    return joint_states(skel, poses, scales, dtype)[:, :, 0:3] * np.asarray(global_scaling, dtype)


def nerr(got, want):
    """Normalised error of an output: max |got - want| / max |want|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


# ------------------------------------------------------------------------------------------------ synthetic skeletons
def make_skeleton(seed, J, V, K, P_pos=104, P_scale=12, parents=None, max_back=6, drive_scale=True):
    """A random skeleton as data (float32 arrays).  parents: an explicit list, or random among the `max_back` preceding joints
    (joint 0 is the root).  Every joint gets 2-4 driven channels; with drive_scale some `sc` channels are driven too (by scale
    parameters and, for a few joints, by a pose parameter).  Vertices have 1..K influences with weights summing to 1."""
    rs = np.random.RandomState(seed)
    if parents is None:
        parents = [-1] + [int(rs.randint(max(0, j - max_back), j)) for j in range(1, J)]
    parents = np.asarray(parents, np.int64)
    q = rs.randn(J, 4)
    pre = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    offset = (rs.randn(J, 3) * 0.3).astype(np.float32)
    P = P_pos + P_scale
    tr = np.zeros((7 * J, P), np.float32)
    for j in range(J):
        for c in rs.choice(6, size=rs.randint(2, 5), replace=False):
            for p in rs.choice(P_pos, size=rs.randint(1, 3), replace=False):
                tr[7 * j + c, p] = rs.uniform(-1, 1) * (0.2 if c < 3 else 1.0)
        if drive_scale and P_scale and rs.rand() < 0.5:
            tr[7 * j + 6, P_pos + rs.randint(P_scale)] = rs.uniform(0.2, 1.0)
        if drive_scale and rs.rand() < 0.1:
            tr[7 * j + 6, rs.randint(P_pos)] = rs.uniform(-0.3, 0.3)
    offs = (rs.randn(7 * J) * 0.05).astype(np.float32)
    offs[6::7] *= 0.2
    rest = rs.randn(V, 3).astype(np.float32)
    idx = np.zeros((V, K), np.int64)
    w = np.zeros((V, K), np.float32)
    for v in range(V):
        n = rs.randint(1, min(K, J) + 1)
        idx[v, :n] = rs.choice(J, size=n, replace=False)
        ww = rs.uniform(0.1, 1.0, n)
        w[v, :n] = (ww / ww.sum()).astype(np.float32)
    return {"parents": parents, "pre_rotation": pre, "joint_offset": offset, "transform": tr, "transform_offsets": offs,
            "skin_indices": idx, "skin_weights": w, "rest_vertices": rest, "nr_position_params": P_pos, "nr_scaling_params": P_scale}


def make_inputs(seed, N, P_pos=104, P_scale=12):
    """(poses [N, P_pos], scales [1, P_scale]) float32: angles of a radian or so, scale exponents of a few tenths."""
    rs = np.random.RandomState(seed)
    return (rs.randn(N, P_pos) * 0.6).astype(np.float32), (rs.randn(1, P_scale) * 0.2).astype(np.float32)


def as_model_dicts(skel):
    """(model_json, lbs_config) holding `skel` the way the reference's files do: bones with Name / Parent / PreRotation /
    TranslationOffset (a root's parent is 2^31, as in the assets), the ragged skinning list (a vertex's non-zero slots in slot
    order) and the dense transform."""
    J, V = np.asarray(skel["parents"]).size, skel["rest_vertices"].shape[0]
    counts = (skel["skin_weights"] > 0).sum(axis=1)
    pairs = [[int(skel["skin_indices"][v, k]), float(skel["skin_weights"][v, k])] for v in range(V) for k in range(counts[v])]
    model = {"Skeleton": {"Bones": [{"Name": f"b{j}", "Parent": int(skel["parents"][j]) if skel["parents"][j] >= 0 else 2 ** 31,
                                     "PreRotation": skel["pre_rotation"][j].tolist(),
                                     "TranslationOffset": skel["joint_offset"][j].tolist()} for j in range(J)]},
             "SkinnedModel": {"RestPositions": skel["rest_vertices"].tolist(), "SkinningWeights": pairs,
                              "SkinningOffsets": np.concatenate([[0], np.cumsum(counts)]).tolist()}}
    cfg = {"transform": skel["transform"], "transform_offsets": np.asarray(skel["transform_offsets"]).reshape(1, -1),
           "nr_scaling_params": int(skel["nr_scaling_params"]), "nr_position_params": int(skel["nr_position_params"])}
    return model, cfg
