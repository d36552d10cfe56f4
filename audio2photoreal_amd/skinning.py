"""Posed body geometry on the MI355X: from un-normalised body poses to a skeleton and a skinned mesh -- the first stage of the
reference's renderer (visualize/ca_body/utils/lbs.py: ParameterTransform, solve_skeleton_state, states_to_matrix,
LinearBlendSkinning.forward, LBSModule.pose), as two HIP launches for all frames (csrc/kernels_skin.h).

    python -m audio2photoreal_amd.skinning --results results.npy --assets static_assets.pt --out geometry.npy [--joints-only]

`BodySkeleton` is built once from the dictionaries the reference reads (`from_model`, `from_static_assets`) or from arrays
(`from_arrays`).  Construction is host work: it packs the ragged skinning list, sorts the joints into depth levels, compresses the
parameter transform to its non-zeros, computes the bind state and its inverse in float64, and rejects anything a kernel could
not index safely.  The methods take poses that live on the GPU and run on the caller's current stream; there is no CPU path.
`joint_loss_grad` and `solve_ik` go the other way -- a loss on joint positions and orientations, its gradient through the skeleton
solve, and descent towards the targets (csrc/kernels_steer.h; sample/steer.py steers a sampler with them).

Poses are the UN-NORMALISED 104 joint parameters: the `"pose"` entry of generate_from_recording / generate_from_long_recording /
generate_conversation / sample.dataset, or the `motions` of a results.npy.  A sampler's raw output [B, 104, 1, T] is normalised:
multiply by pose_std and add pose_mean first (sample.generate.make_inv_transform)."""
from __future__ import annotations

import argparse
import ctypes as C
import sys
from typing import Optional

import numpy as np
import torch

from . import _lib, avatar
from ._lib import A2PError

CHANNELS = 7   # tx ty tz rx ry rz sc per joint


# ------------------------------------------------------------------------------------------------ host preparation
def pack_skinning(indices, weights, offsets, num_max_skin_joints: int = 8):
    """The ragged skinning list (influence e of vertex v at offsets[v] + e) -> [V, K] index (int64) and weight (float32) tables
    by the reference's rule: the first K influences are kept, the rest dropped, nothing renormalised; unused slots are 0 / 0."""
    K = int(num_max_skin_joints)
    indices, weights = np.asarray(indices).reshape(-1), np.asarray(weights, np.float32).reshape(-1)
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    if K < 1:
        raise ValueError(f"num_max_skin_joints must be >= 1 (got {K})")
    if offsets.size < 2:
        raise ValueError("SkinningOffsets needs at least two entries (one vertex)")
    if indices.size != weights.size:
        raise ValueError(f"skinning indices ({indices.size}) and weights ({weights.size}) differ in length")
    bad = np.nonzero((np.diff(offsets) < 0))[0]
    if bad.size or offsets[0] < 0 or offsets[-1] > indices.size:
        where = f"SkinningOffsets[{int(bad[0]) + 1}]" if bad.size else "SkinningOffsets"
        raise ValueError(f"{where} is not an ascending range inside the {indices.size} skinning entries")
    V = offsets.size - 1
    idx = np.zeros((V, K), np.int64)
    w = np.zeros((V, K), np.float32)
    for k in range(K):
        src = offsets[:-1] + k
        has = src < offsets[1:]
        idx[has, k] = indices[src[has]]
        w[has, k] = weights[src[has]]
    return idx, w


def normalise_parents(parents) -> np.ndarray:
    """[J] int64 with -1 for every root: a parent that is negative or >= J marks a root (several roots are allowed)."""
    p = np.asarray(parents, np.int64).reshape(-1).copy()
    p[(p < 0) | (p >= p.size)] = -1
    return p


def level_schedule(parents):
    """(order [J], level_start [L + 1], depth [J]): the joints sorted by depth (ascending index inside a level); level l is
    order[level_start[l]:level_start[l + 1]], level 0 the roots, and every joint sits one level after its parent.  A parent that
    does not precede its child is rejected (the reference's joint loop cannot run it either)."""
    p = normalise_parents(parents)
    depth = np.zeros(p.size, np.int64)
    for j in range(p.size):
        if p[j] >= j:
            raise ValueError(f"joint {j}: parent {int(p[j])} does not precede it")
        if p[j] >= 0:
            depth[j] = depth[p[j]] + 1
    order = np.argsort(depth, kind="stable")
    level_start = np.concatenate([[0], np.cumsum(np.bincount(depth))])
    return order.astype(np.int64), level_start.astype(np.int64), depth


def child_list(parents):
    """(child_ptr [J + 1], child_idx): the children of joint j are child_idx[child_ptr[j]:child_ptr[j + 1]], ascending -- the
    order in which the backward pass of the skeleton solve sums their adjoints (csrc/kernels_steer.h)."""
    p = normalise_parents(parents)
    kids = np.nonzero(p >= 0)[0]
    kids = kids[np.argsort(p[kids], kind="stable")]
    child_ptr = np.concatenate([[0], np.cumsum(np.bincount(p[kids], minlength=p.size))])
    return child_ptr.astype(np.int64), kids.astype(np.int64)


def compress_columns(transform, n_cols: int):
    """The first n_cols columns of the dense [R, P] transform as compressed columns (col_ptr [n_cols + 1], rows, vals float32),
    rows ascending inside a column: the transposed parameter transform, one output per column."""
    t = np.asarray(transform, np.float32)[:, :n_cols]
    cols, rows = np.nonzero(t.T)
    col_ptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n_cols))])
    return col_ptr.astype(np.int64), rows.astype(np.int64), t[rows, cols]


def compress_transform(transform):
    """Dense [R, P] -> compressed rows (row_ptr [R + 1], cols, vals float32), columns ascending inside a row."""
    t = np.asarray(transform, np.float32)
    rows, cols = np.nonzero(t)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=t.shape[0]))])
    return row_ptr.astype(np.int64), cols.astype(np.int64), t[rows, cols]


def apply_compressed(row_ptr, cols, vals, x):
    """x [N, P] -> [N, R] through the compressed rows, in float64 (host check of compress_transform)."""
    x = np.asarray(x, np.float64)
    out = np.zeros((x.shape[0], row_ptr.size - 1))
    for r in range(row_ptr.size - 1):
        e = slice(row_ptr[r], row_ptr[r + 1])
        out[:, r] = x[:, cols[e]] @ vals[e].astype(np.float64)
    return out


def _qmul(q, r):
    return np.array([q[3] * r[0] + q[0] * r[3] + q[1] * r[2] - q[2] * r[1], q[3] * r[1] - q[0] * r[2] + q[1] * r[3] + q[2] * r[0],
                     q[3] * r[2] + q[0] * r[1] - q[1] * r[0] + q[2] * r[3], q[3] * r[3] - q[0] * r[0] - q[1] * r[1] - q[2] * r[2]])


def _qrot(q, v):
    av = np.cross(q[:3], v)
    return v + 2.0 * (av * q[3] + np.cross(q[:3], av))


def bind_state64(parents, pre_rotation, joint_offset, transform_offsets):
    """(bind [J, 8], inverse [J, 8]) in float64: the states of the all-zero parameter vector (the joint values are the transform
    offsets), and per joint (rot(q^-1, -t) / s, q^-1, 1 / s) -- what states_to_matrix multiplies every frame's state with."""
    p = normalise_parents(parents)
    J = p.size
    val = np.asarray(transform_offsets, np.float64).reshape(J, CHANNELS)
    pre, off = np.asarray(pre_rotation, np.float64), np.asarray(joint_offset, np.float64)
    bind, inv = np.zeros((J, 8)), np.zeros((J, 8))
    with np.errstate(all="ignore"):          # a degenerate bind state comes out non-finite and is rejected by the caller
        for j in range(J):
            h = val[j, 3:6] * np.array([-0.5, 0.5, 0.5])
            c, s = np.cos(h), np.sin(h)
            e = np.array([-s[0] * c[1] * c[2] - c[0] * s[1] * s[2], c[0] * s[1] * c[2] - s[0] * c[1] * s[2],
                          c[0] * c[1] * s[2] + s[0] * s[1] * c[2], c[0] * c[1] * c[2] - s[0] * s[1] * s[2]])
            t, q, sc = val[j, 0:3] + off[j], _qmul(pre[j], e), np.exp2(val[j, 6])
            if p[j] >= 0:
                b = bind[p[j]]
                t, q, sc = _qrot(b[3:7], t * b[7]) + b[0:3], _qmul(b[3:7], q), b[7] * sc
            bind[j, 0:3], bind[j, 3:7], bind[j, 7] = t, q, sc
            qi = q * np.array([-1.0, -1.0, -1.0, 1.0]) / np.dot(q, q)
            inv[j, 0:3], inv[j, 3:7], inv[j, 7] = _qrot(qi, -t) / sc, qi, 1.0 / sc
    return bind, inv


def _finite(name: str, a):
    a = np.asarray(a)
    bad = np.argwhere(~np.isfinite(a))
    if bad.size:
        raise ValueError(f"{name}{list(map(int, bad[0]))} is not finite ({a[tuple(bad[0])]})")


def motion_frames(motion, n_params: int = 104):
    """(frames [N, n_params], lead): the accepted pose layouts as flat frames.  [B, T, P] (the generators' "pose") -> lead (B, T);
    [B, P, 1, T] (sampler layout, un-normalised by the caller) -> lead (B, T), frame (b, t) = motion[b, :, 0, t]; [N, P] -> lead
    (N,).  numpy or tensor; the result is the same kind, float32."""
    is_t = torch.is_tensor(motion)
    if not (is_t or isinstance(motion, np.ndarray)):
        raise A2PError(f"motion must be a tensor or an ndarray (got {type(motion).__name__})")
    shape = tuple(motion.shape)
    if len(shape) == 4 and shape[2] == 1 and shape[1] == n_params:
        m = motion.permute(0, 3, 1, 2) if is_t else motion.transpose(0, 3, 1, 2)
        lead = (shape[0], shape[3])
    elif len(shape) == 3 and shape[2] == n_params:
        m, lead = motion, shape[:2]
    elif len(shape) == 2 and shape[1] == n_params:
        m, lead = motion, shape[:1]
    else:
        raise A2PError(f"motion must be [B, T, {n_params}], [B, {n_params}, 1, T] or [N, {n_params}] (got {list(shape)})")
    m = m.reshape(-1, n_params)
    return (m.to(torch.float32).contiguous() if is_t else np.ascontiguousarray(m, np.float32)), tuple(int(v) for v in lead)


# ------------------------------------------------------------------------------------------------ joint constraints
REACH, AIM = _lib.STEER_REACH, _lib.STEER_AIM


class JointConstraints:
    """K <= 16 constraints on N frames, as the steer kernel reads them (include/a2p_hip.h a2p_steer): host lists `joints` [K]
    (indices), `kinds` [K] (REACH / AIM) and `axes` [K, 3] (the unit axis of an aim in the joint's frame; ignored by a reach), and
    `targets` [N, K, 3] / `weights` [N, K] (float32; numpy, or tensors on any device).  Targets are in the units of
    pose_motion's "joints": translation times global_scaling.  Host data is validated here; sample.steer.JointTargets builds these."""

    def __init__(self, joints, kinds, axes, targets, weights, n_joints: Optional[int] = None):
        self.joints = [int(j) for j in joints]
        self.kinds = [int(k) for k in kinds]
        self.axes = np.ascontiguousarray(axes, np.float32).reshape(-1, 3)
        K = len(self.joints)
        if K < 1 or K > _lib.STEER_MAX_CONSTRAINTS:
            raise A2PError(f"{K} constraints: the steer kernel takes 1..{_lib.STEER_MAX_CONSTRAINTS}")
        if len(self.kinds) != K or self.axes.shape[0] != K:
            raise A2PError(f"joints ({K}), kinds ({len(self.kinds)}) and axes ({self.axes.shape[0]}) differ in length")
        for k in range(K):
            if self.kinds[k] not in (REACH, AIM):
                raise A2PError(f"constraint {k}: kind {self.kinds[k]} is neither REACH ({REACH}) nor AIM ({AIM})")
            if self.joints[k] < 0 or (n_joints is not None and self.joints[k] >= n_joints):
                raise A2PError(f"constraint {k}: joint {self.joints[k]} is outside [0, {n_joints})")
            if self.kinds[k] == AIM:
                check_axis(self.axes[k], f"constraint {k}")
        as_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, np.float32))
        self.targets, self.weights = as_t(targets).to(torch.float32), as_t(weights).to(torch.float32)
        N = self.weights.shape[0]
        if tuple(self.targets.shape) != (N, K, 3) or tuple(self.weights.shape) != (N, K):
            raise A2PError(f"targets must be [N, {K}, 3] and weights [N, {K}] (got {list(self.targets.shape)}, {list(self.weights.shape)})")
        if not self.weights.is_cuda:
            w = self.weights.numpy()
            if not (np.isfinite(w).all() and (w >= 0).all()):
                raise A2PError("weights must be finite and >= 0")
        if not self.targets.is_cuda and not bool(torch.isfinite(self.targets).all()):
            raise A2PError("targets must be finite")
        self.N, self.K = int(N), K

    def on(self, device):
        """(targets, weights) contiguous on `device`."""
        return self.targets.to(device).contiguous(), self.weights.to(device).contiguous()


def check_axis(axis, what: str) -> np.ndarray:
    """A finite unit 3-vector (|axis| within 1e-4 of 1), or A2PError."""
    a = np.asarray(axis, np.float64).reshape(-1)
    if a.size != 3 or not np.isfinite(a).all() or abs(float(np.linalg.norm(a)) - 1.0) > 1e-4:
        raise A2PError(f"{what}: axis {a.tolist()} is not a finite unit 3-vector")
    return a.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the skeleton
class BodySkeleton:
    """A skinned skeleton, validated and laid out for the kernels.  Host arrays live on the object; device copies are made on
    first use, per device."""

    def __init__(self):
        raise TypeError("use BodySkeleton.from_model, .from_static_assets or .from_arrays")

    @classmethod
    def from_arrays(cls, parents, pre_rotation, joint_offset, transform, transform_offsets, nr_position_params: int,
                    nr_scaling_params: int, rest_vertices, skin_indices, skin_weights, template_verts=None, lbs_scale=None,
                    global_scaling=None, joint_names=None) -> "BodySkeleton":
        """parents [J]; pre_rotation [J, 4] xyzw; joint_offset [J, 3]; transform [7 J, P_pos + P_scale]; transform_offsets [7 J];
        rest_vertices [V, 3]; skin_indices / skin_weights [V, K] (packed: pack_skinning); template_verts [V, 3], lbs_scale
        [P_scale] and global_scaling (scalar or [3]) are LBSModule's extras."""
        self = object.__new__(cls)
        raw_parents = np.asarray(parents, np.int64).reshape(-1)
        J = raw_parents.size
        if J < 1 or J > _lib.SKIN_MAX_JOINTS:
            raise ValueError(f"the skeleton has J={J} joints; the kernels take 1..{_lib.SKIN_MAX_JOINTS}")
        self.parents = normalise_parents(raw_parents)
        self.order, self.level_start, self.depth = level_schedule(self.parents)
        self.pre_rotation = np.ascontiguousarray(pre_rotation, np.float32).reshape(-1, 4)
        self.joint_offset = np.ascontiguousarray(joint_offset, np.float32).reshape(-1, 3)
        if self.pre_rotation.shape[0] != J or self.joint_offset.shape[0] != J:
            raise ValueError(f"pre_rotation {self.pre_rotation.shape} / joint_offset {self.joint_offset.shape} do not hold J={J} joints")
        self.P_pos, self.P_scale = int(nr_position_params), int(nr_scaling_params)
        P = self.P_pos + self.P_scale
        if self.P_pos < 1 or self.P_scale < 0 or P > _lib.SKIN_MAX_PARAMS:
            raise ValueError(f"nr_position_params={self.P_pos}, nr_scaling_params={self.P_scale}: need >= 1, >= 0 and a sum <= {_lib.SKIN_MAX_PARAMS}")
        self.transform = np.ascontiguousarray(transform, np.float32)
        if self.transform.shape != (CHANNELS * J, P):
            raise ValueError(f"transform is {list(self.transform.shape)}; expected [7 J, P] = [{CHANNELS * J}, {P}]")
        self.transform_offsets = np.ascontiguousarray(transform_offsets, np.float32).reshape(-1)
        if self.transform_offsets.size != CHANNELS * J:
            raise ValueError(f"transform_offsets holds {self.transform_offsets.size} values; expected 7 J = {CHANNELS * J}")
        self.rest_vertices = np.ascontiguousarray(rest_vertices, np.float32).reshape(-1, 3)
        V = self.rest_vertices.shape[0]
        idx = np.asarray(skin_indices)
        self.skin_weights = np.ascontiguousarray(skin_weights, np.float32)
        if idx.ndim != 2 or idx.shape != self.skin_weights.shape or idx.shape[0] != V or V < 1:
            raise ValueError(f"skin_indices {list(idx.shape)} / skin_weights {list(self.skin_weights.shape)} must both be [V={V}, K]")
        K = idx.shape[1]
        if K < 1 or K > _lib.SKIN_MAX_INFLUENCES:
            raise ValueError(f"K={K} influences per vertex; the kernels take 1..{_lib.SKIN_MAX_INFLUENCES}")
        bad = np.argwhere((idx < 0) | (idx >= J))
        if bad.size:
            v, k = map(int, bad[0])
            raise ValueError(f"skin_indices[{v}, {k}] = {int(idx[v, k])} is outside [0, J={J})")
        self.skin_indices = np.ascontiguousarray(idx, np.int64)
        self.template_verts = None if template_verts is None else np.ascontiguousarray(
            torch.as_tensor(template_verts).detach().cpu().numpy(), np.float32).reshape(-1, 3)
        if self.template_verts is not None and self.template_verts.shape[0] != V:
            raise ValueError(f"template_verts holds {self.template_verts.shape[0]} vertices; the skin has V={V}")
        self.lbs_scale = None if lbs_scale is None else np.ascontiguousarray(
            torch.as_tensor(lbs_scale).detach().cpu().numpy(), np.float32).reshape(-1)
        if self.lbs_scale is not None and self.lbs_scale.size != self.P_scale:
            raise ValueError(f"lbs_scale holds {self.lbs_scale.size} values; nr_scaling_params={self.P_scale}")
        g = np.ones(3, np.float32) if global_scaling is None else np.asarray(
            torch.as_tensor(global_scaling).detach().cpu().numpy(), np.float32).reshape(-1)
        if g.size not in (1, 3):
            raise ValueError(f"global_scaling must be a scalar or [3] (got {g.size} values)")
        self.global_scaling = np.broadcast_to(g, (3,)).copy()
        for name, a in (("pre_rotation", self.pre_rotation), ("joint_offset", self.joint_offset), ("transform", self.transform),
                        ("transform_offsets", self.transform_offsets), ("rest_vertices", self.rest_vertices),
                        ("skin_weights", self.skin_weights), ("template_verts", self.template_verts), ("lbs_scale", self.lbs_scale),
                        ("global_scaling", self.global_scaling)):
            if a is not None:
                _finite(name, a)
        self.joint_names = list(joint_names) if joint_names is not None else [f"joint{j}" for j in range(J)]
        self.J, self.V, self.K = J, V, K
        self.row_ptr, self.cols, self.vals = compress_transform(self.transform)
        self.col_ptr, self.col_rows, self.col_vals = compress_columns(self.transform, self.P_pos)
        self.child_ptr, self.child_idx = child_list(self.parents)
        self.bind_state, self.inv_bind = bind_state64(self.parents, self.pre_rotation, self.joint_offset, self.transform_offsets)
        _finite("bind_state", self.bind_state)
        _finite("inverse bind state", self.inv_bind)
        self._dev = {}
        return self

    @classmethod
    def from_model(cls, model_json: dict, lbs_config: dict, num_max_skin_joints: int = 8, template_verts=None, lbs_scale=None,
                   global_scaling=None) -> "BodySkeleton":
        """The two dictionaries of the reference's LinearBlendSkinning.__init__ (plus LBSModule's extras)."""
        if num_max_skin_joints > _lib.SKIN_MAX_INFLUENCES:
            raise ValueError(f"num_max_skin_joints={num_max_skin_joints}: K is at most {_lib.SKIN_MAX_INFLUENCES}")
        bones = model_json["Skeleton"]["Bones"]
        skin = model_json["SkinnedModel"]
        pairs = skin["SkinningWeights"]
        idx, w = pack_skinning([e[0] for e in pairs], [e[1] for e in pairs], skin["SkinningOffsets"], num_max_skin_joints)
        as_np = lambda a: torch.as_tensor(a).detach().cpu().numpy()
        return cls.from_arrays(
            [b["Parent"] for b in bones], [b["PreRotation"] for b in bones], [b["TranslationOffset"] for b in bones],
            as_np(lbs_config["transform"]), as_np(lbs_config["transform_offsets"]), lbs_config["nr_position_params"],
            lbs_config["nr_scaling_params"], skin["RestPositions"], idx, w, template_verts=template_verts, lbs_scale=lbs_scale,
            global_scaling=global_scaling, joint_names=[b["Name"] for b in bones])

    @classmethod
    def from_static_assets(cls, assets) -> "BodySkeleton":
        """The mapping the reference's BodyRenderer loads from static_assets.pt."""
        return cls.from_model(assets["lbs_model_json"], assets["lbs_config_dict"], template_verts=assets["lbs_template_verts"],
                              lbs_scale=assets["lbs_scale"], global_scaling=assets["global_scaling"])

    # -------------------------------------------------------------------------------------------- device side
    def _tables(self, device):
        key = str(device)
        if key not in self._dev:
            i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(device)
            f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
            base = self.rest_vertices if self.template_verts is None else self.template_verts
            self._dev[key] = {
                "row_ptr": i32(self.row_ptr), "cols": i32(self.cols), "vals": f32(self.vals), "offsets": f32(self.transform_offsets),
                "joint_offset": f32(self.joint_offset), "pre_rotation": f32(self.pre_rotation), "parents": i32(self.parents),
                "order": i32(self.order), "level_start": i32(self.level_start), "inv_bind": f32(self.inv_bind),
                "child_ptr": i32(self.child_ptr), "child_idx": i32(self.child_idx if self.child_idx.size else [0]),
                "col_ptr": i32(self.col_ptr), "col_rows": i32(self.col_rows if self.col_rows.size else [0]),
                "col_vals": f32(self.col_vals if self.col_vals.size else [0]),
                "idx": i32(self.skin_indices.T), "w": f32(self.skin_weights.T),             # [K, V]: a wave reads consecutive entries
                "base": f32(base), "lbs_scale": None if self.lbs_scale is None else f32(self.lbs_scale.reshape(1, -1))}
        return self._dev[key]

    def _inputs(self, poses, scales):
        if not torch.is_tensor(poses):
            raise A2PError(f"poses must be a tensor on the MI355X (got {type(poses).__name__})")
        _lib.require_gpu_tensor(poses, "poses")
        if poses.dim() != 2 or poses.shape[1] != self.P_pos:
            raise A2PError(f"poses must be [N, {self.P_pos}] (got {list(poses.shape)})")
        poses = poses.to(torch.float32).contiguous()
        t = self._tables(poses.device)
        N = poses.shape[0]
        if self.P_scale == 0:
            return poses, None, 0, t
        if scales is None:
            if t["lbs_scale"] is None:
                raise A2PError(f"scales is None and the skeleton has no lbs_scale: pass scales [N or 1, {self.P_scale}]")
            scales = t["lbs_scale"]
        else:
            if not torch.is_tensor(scales):
                raise A2PError(f"scales must be a tensor on the MI355X (got {type(scales).__name__})")
            _lib.require_gpu_tensor(scales, "scales")
            if scales.device != poses.device:
                raise A2PError(f"scales is on {scales.device}, poses on {poses.device}")
            if scales.dim() != 2 or scales.shape[1] != self.P_scale or scales.shape[0] not in (1, N):
                raise A2PError(f"scales must be [{N} or 1, {self.P_scale}] (got {list(scales.shape)})")
            scales = scales.to(torch.float32).contiguous()
        return poses, scales, int(scales.shape[0] == N and N != 1), t

    def _solve(self, poses, scales, want_states: bool, want_mats: bool):
        poses, scales, per_frame, t = self._inputs(poses, scales)
        N, dev = poses.shape[0], poses.device
        states = torch.empty(N, self.J, 8, dtype=torch.float32, device=dev) if want_states else None
        mats = torch.empty(N, self.J, 3, 4, dtype=torch.float32, device=dev) if want_mats else None
        lib = _lib.load()
        with _lib.on_device_of(poses):
            _lib.check(lib.a2p_skin_states(
                _lib.ptr(poses), _lib.ptr(scales), per_frame, N, self.P_pos, self.P_scale, self.J, _lib.ptr(t["row_ptr"]),
                _lib.ptr(t["cols"]), _lib.ptr(t["vals"]), _lib.ptr(t["offsets"]), _lib.ptr(t["joint_offset"]),
                _lib.ptr(t["pre_rotation"]), _lib.ptr(t["parents"]), _lib.ptr(t["order"]), _lib.ptr(t["level_start"]),
                self.level_start.size - 1, _lib.ptr(t["inv_bind"]), _lib.ptr(states), _lib.ptr(mats), _lib.current_stream(dev)),
                "a2p_skin_states")
        return states, mats, t

    def joint_states(self, poses, scales=None):
        """[N, J, 8]: translation 3, quaternion xyzw 4, scale 1 (solve_skeleton_state)."""
        return self._solve(poses, scales, True, False)[0]

    def transforms(self, poses, scales=None):
        """[N, J, 3, 4] = states_to_matrix(bind_state, states): [R s | t], indexed [frame, joint, row, column]."""
        return self._solve(poses, scales, False, True)[1]

    def joint_positions(self, poses, scales=None):
        """[N, J, 3]: the state translations times global_scaling."""
        states = self.joint_states(poses, scales)
        return states[:, :, 0:3] * torch.from_numpy(self.global_scaling).to(states.device)

    # -------------------------------------------------------------------------------------------- steering
    def steer_description(self, t, cons: "JointConstraints", targets, weights, mean, std, scales, per_frame: int, alpha: float,
                          iterations: int, max_step: float):
        """(a2p_steer, keep-alive tuple) for a library call: `t` the device tables, targets / weights / mean / std / scales
        contiguous fp32 tensors on that device (mean / std / scales may be None)."""
        if not isinstance(cons, JointConstraints):
            raise A2PError(f"constraints must be JointConstraints (got {type(cons).__name__})")
        if max(cons.joints) >= self.J:
            raise A2PError(f"constraint joint {max(cons.joints)} is outside [0, J={self.J})")
        iterations = int(iterations)
        if iterations < 0 or iterations > 1024:
            raise A2PError(f"iterations must be in [0, 1024] (got {iterations})")
        if not (np.isfinite(alpha) and alpha > 0 and np.isfinite(max_step) and max_step > 0):
            raise A2PError(f"alpha ({alpha}) and max_step ({max_step}) must be positive and finite")
        K = cons.K
        joints, kinds = (C.c_int32 * K)(*cons.joints), (C.c_int32 * K)(*cons.kinds)
        axes = (C.c_float * (3 * K))(*[float(v) for v in cons.axes.reshape(-1)])
        d = _lib.A2PSteer()
        for name, key in (("row_ptr", "row_ptr"), ("cols", "cols"), ("vals", "vals"), ("offsets", "offsets"),
                          ("joint_offset", "joint_offset"), ("pre_rotation", "pre_rotation"), ("parents", "parents"), ("order", "order"),
                          ("level_start", "level_start"), ("child_ptr", "child_ptr"), ("child_idx", "child_idx"), ("col_ptr", "col_ptr"),
                          ("rows", "col_rows"), ("cvals", "col_vals")):
            setattr(d, name, _lib.ptr(t[key]))
        d.mean, d.std, d.scale = _lib.ptr(mean), _lib.ptr(std), _lib.ptr(scales)
        d.joints_host, d.kinds_host, d.axes_host = joints, kinds, axes
        d.targets, d.weights = _lib.ptr(targets), _lib.ptr(weights)
        d.global_scaling = (C.c_float * 3)(*[float(v) for v in self.global_scaling])
        d.alpha, d.max_step = float(alpha), float(max_step)
        d.P_pos, d.P_scale, d.J, d.n_levels = self.P_pos, self.P_scale, self.J, self.level_start.size - 1
        d.scale_per_frame, d.K, d.iterations = int(per_frame), K, iterations
        return d, (joints, kinds, axes, targets, weights, mean, std, scales)

    def _steer(self, poses, cons, scales, mean, std, iterations, alpha, max_step, want_grad: bool):
        poses, scales, per_frame, t = self._inputs(poses, scales)
        N, dev = poses.shape[0], poses.device
        if not isinstance(cons, JointConstraints):
            raise A2PError(f"constraints must be JointConstraints (got {type(cons).__name__})")
        if cons.N != N:
            raise A2PError(f"the constraints cover {cons.N} frames, poses {N}")
        stat = []
        for name, v in (("mean", mean), ("std", std)):
            if v is not None:
                v = torch.as_tensor(v, dtype=torch.float32).reshape(-1).to(dev).contiguous()
                if v.numel() != self.P_pos:
                    raise A2PError(f"{name} must hold P_pos = {self.P_pos} values (got {v.numel()})")
            stat.append(v)
        targets, weights = cons.on(dev)
        d, keep = self.steer_description(t, cons, targets, weights, stat[0], stat[1], scales, per_frame, alpha, iterations, max_step)
        out = torch.empty_like(poses)
        loss = torch.empty(N, dtype=torch.float32, device=dev)
        grad = torch.empty(N, self.P_pos, dtype=torch.float32, device=dev) if want_grad else None
        with _lib.on_device_of(poses):
            _lib.check(_lib.load().a2p_skin_steer(C.byref(d), _lib.ptr(poses), self.P_pos, N, _lib.ptr(out), self.P_pos, _lib.ptr(loss),
                                                  _lib.ptr(grad), _lib.current_stream(dev)), "a2p_skin_steer")
        del keep
        return out, loss, grad

    def joint_loss_grad(self, poses, constraints, scales=None, mean=None, std=None):
        """(loss [N], grad [N, P_pos]) of the constraints at `poses` [N, P_pos] (include/a2p_hip.h a2p_skin_steer with
        iterations = 0): reach w/2 |p - y|^2, aim w (1 - rot(q, axis) . d), summed over the constraints of a frame, and the
        gradient with respect to the poses -- or, with `mean` / `std` [P_pos], with respect to z where pose = mean + std z and
        `poses` holds z.  The scale parameters are constants."""
        _, loss, grad = self._steer(poses, constraints, scales, mean, std, 0, 1.0, 1.0, True)
        return loss, grad

    def solve_ik(self, poses, constraints, iterations: int = 2, alpha: float = 1.0, max_step: float = 0.25, scales=None, mean=None,
                 std=None):
        """Poses [N, P_pos] moved towards the constraints by `iterations` steps of z <- z - min(alpha L / |g|^2, max_step / |g|inf) g
        (Polyak's step under a trust region; a2p_skin_steer).  With `mean` / `std` the descent runs in the z-scored space
        (`poses` holds z, and max_step is in standard deviations); without them in the pose parameters themselves.  Frames
        whose weights are all zero, and frames whose loss or gradient is zero or not finite, come back unchanged."""
        return self._steer(poses, constraints, scales, mean, std, iterations, alpha, max_step, False)[0]

    def skin(self, mats, verts_unposed=None):
        """[N, V, 3] from skinning matrices [N, J, 3, 4] (what `transforms` returns): LBSModule.pose after the skeleton solve."""
        if not torch.is_tensor(mats):
            raise A2PError(f"mats must be a tensor on the MI355X (got {type(mats).__name__})")
        _lib.require_gpu_tensor(mats, "mats")
        if mats.dim() != 4 or tuple(mats.shape[1:]) != (self.J, 3, 4) or mats.dtype != torch.float32:
            raise A2PError(f"mats must be float32 [N, {self.J}, 3, 4] (got {mats.dtype} {list(mats.shape)})")
        mats = mats.contiguous()
        N, dev = mats.shape[0], mats.device
        t = self._tables(dev)
        per_frame = 0
        if verts_unposed is not None:
            if not torch.is_tensor(verts_unposed):
                raise A2PError(f"verts_unposed must be a tensor on the MI355X (got {type(verts_unposed).__name__})")
            _lib.require_gpu_tensor(verts_unposed, "verts_unposed")
            if verts_unposed.device != dev:
                raise A2PError(f"verts_unposed is on {verts_unposed.device}, poses on {dev}")
            shape = tuple(verts_unposed.shape)
            if shape not in ((self.V, 3), (1, self.V, 3), (N, self.V, 3)):
                raise A2PError(f"verts_unposed must be [{self.V}, 3], [1, {self.V}, 3] or [{N}, {self.V}, 3] (got {list(shape)})")
            per_frame = int(len(shape) == 3 and shape[0] == N and N != 1)
            verts_unposed = verts_unposed.to(torch.float32).contiguous()
        out = torch.empty(N, self.V, 3, dtype=torch.float32, device=dev)
        g = self.global_scaling
        lib = _lib.load()
        with _lib.on_device_of(mats):
            _lib.check(lib.a2p_skin_vertices(_lib.ptr(mats), N, self.J, _lib.ptr(t["base"]), _lib.ptr(verts_unposed), per_frame,
                                             _lib.ptr(t["idx"]), _lib.ptr(t["w"]), self.V, self.K, float(g[0]), float(g[1]), float(g[2]),
                                             _lib.ptr(out), _lib.current_stream(dev)), "a2p_skin_vertices")
        return out

    def pose_vertices(self, poses, scales=None, verts_unposed=None):
        """[N, V, 3] = LBSModule.pose: skin (verts_unposed + template_verts) and multiply by global_scaling.  Without
        verts_unposed the template vertices are skinned (the rest vertices when the skeleton has no template).  verts_unposed:
        [V, 3], [1, V, 3] or [N, V, 3]."""
        return self.skin(self._solve(poses, scales, False, True)[1], verts_unposed)

    def unpose_vertices(self, poses, verts, scales=None):
        """[N, V, 3] = LBSModule.unpose: the displacement from the template (the rest vertices when the skeleton has no template)
        that pose_vertices maps to `verts` [N, V, 3]: verts / global_scaling goes through the inverse of each vertex's blended
        skinning matrix and the template is subtracted.  The inverse is the closed-form adjugate over the determinant in fp32 (the
        reference calls Tensor.inverse() on the 4 x 4 matrix).  A singular or non-finite blend gives a non-finite result: the
        output is checked once per call, and A2PError names the first bad frame and vertex."""
        mats, t = self._solve(poses, scales, False, True)[1:]
        N, dev = mats.shape[0], mats.device
        if not torch.is_tensor(verts):
            raise A2PError(f"verts must be a tensor on the MI355X (got {type(verts).__name__})")
        _lib.require_gpu_tensor(verts, "verts")
        if verts.device != dev:
            raise A2PError(f"verts is on {verts.device}, poses on {dev}")
        if tuple(verts.shape) != (N, self.V, 3) or verts.dtype != torch.float32:
            raise A2PError(f"verts must be float32 [{N}, {self.V}, 3] (got {verts.dtype} {list(verts.shape)})")
        verts = verts.contiguous()
        out = torch.empty(N, self.V, 3, dtype=torch.float32, device=dev)
        g = self.global_scaling
        with _lib.on_device_of(mats):
            _lib.check(_lib.load().a2p_unskin_vertices(_lib.ptr(mats), N, self.J, _lib.ptr(verts), _lib.ptr(t["base"]), _lib.ptr(t["idx"]),
                                                       _lib.ptr(t["w"]), self.V, self.K, float(g[0]), float(g[1]), float(g[2]),
                                                       _lib.ptr(out), _lib.current_stream(dev)), "a2p_unskin_vertices")
        finite = torch.isfinite(out)
        if not bool(finite.all()):
            n, v = (int(i) for i in torch.nonzero(~finite.all(dim=2))[0])
            raise A2PError(f"unpose_vertices: frame {n}, vertex {v} is not finite: its blended skinning matrix is singular or not "
                           "finite (or verts is not finite there)")
        return out


# ------------------------------------------------------------------------------------------------ convenience
def pose_motion(skeleton: BodySkeleton, motion, vertices: bool = True, device=None) -> dict:
    """{"joints": [B, T, J, 3], "vertices": [B, T, V, 3]} (float32 tensors on the GPU) of un-normalised body motion: the "pose"
    entry the generators return [B, T, 104] (numpy or tensor), the sampler layout [B, 104, 1, T] -- UN-NORMALISED first, see the
    module docstring -- or flat frames [N, 104] (then the outputs are [N, J, 3] / [N, V, 3]).  The scales are the skeleton's
    lbs_scale.  vertices=False skips the mesh.  A numpy input goes to `device` (default: the current GPU)."""
    frames, lead = avatar.clip_frames("pose_motion", motion, skeleton.P_pos, device)
    g = torch.from_numpy(skeleton.global_scaling).to(frames.device)
    if not vertices:
        return {"joints": (skeleton.joint_states(frames)[:, :, 0:3] * g).reshape(*lead, skeleton.J, 3)}
    states, mats, _ = skeleton._solve(frames, None, True, True)
    return {"joints": (states[:, :, 0:3] * g).reshape(*lead, skeleton.J, 3),
            "vertices": skeleton.skin(mats).reshape(*lead, skeleton.V, 3)}


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m audio2photoreal_amd.skinning",
                                 description="Pose the body mesh for the motions of a results.npy (un-normalised body poses).")
    ap.add_argument("--results", required=True, help="results.npy of sample.generate (key `motions` [B, 104, 1, T])")
    ap.add_argument("--assets", required=True, help="static_assets.pt: lbs_model_json, lbs_config_dict, lbs_template_verts, lbs_scale, global_scaling")
    ap.add_argument("--out", required=True, help="geometry.npy: a pickled dict of float32 arrays `joints` (and `vertices`)")
    ap.add_argument("--joints-only", action="store_true", help="skip the mesh")
    return ap


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    (motions,) = avatar.load_block(args.results, ("motions", "motion"))
    skeleton = BodySkeleton.from_static_assets(torch.load(args.assets, map_location="cpu", weights_only=False))
    out = pose_motion(skeleton, np.asarray(motions), vertices=not args.joints_only)
    np.save(args.out, {k: v.cpu().numpy() for k, v in out.items()})
    print(f"{args.out}: " + ", ".join(f"{k} {list(v.shape)}" for k, v in out.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
