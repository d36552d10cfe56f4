"""Several bodies in one image on the MI355X: both people of a conversation in one world, with one z-buffer per sample, so that
they occlude each other correctly along anti-aliased silhouettes (csrc/kernels_scene.h; INTEGRATION.md "Two people in one scene").

    python -m audio2photoreal_amd.scene --results a.npy b.npy --assets A/static_assets.pt B/static_assets.pt
                                        --checkpoint A/body_dec.ckpt B/body_dec.ckpt --yaw 25 -25 --position x y z x y z --out frames.npy
                                        [--up x y z] [--pivot x y z x y z] [--video clip.avi --audio conversation.wav] [--supersample 2]
                                        [--background R G B] [--size H W] [--camera-json FILE | --eye x y z --target x y z --fov deg]

`SceneRasterizer` holds 1 to 4 mesh topologies and an image size; `render` takes each body's vertices, texture and optional rigid
placement and returns the image, its coverage, its depth and each body's share of every pixel.  `render_conversation_motion` and
`render_conversation_video` run the whole chain per person -- encode, decode, pose, texture -- and render the people together.
Cameras are OpenCV pinholes as in render.py; all tensors are float32 on the GPU; there is no CPU path."""
from __future__ import annotations

import argparse
import copy
import sys

import numpy as np
import torch

from . import _lib, avatar
from ._lib import A2PError
from .avatar import Avatar, load_avatar  # noqa: F401  (this module's names for them)
from .render import BodyRasterizer, RenderArguments
from .surface import BodySurface

MAX_BODIES = _lib.SCENE_MAX_BODIES
RIGID_TOLERANCE = 1e-4                      # |R R^T - I| of a placement render_conversation_motion accepts


def placement(yaw_degrees: float, position, up, pivot=(0.0, 0.0, 0.0), device=None):
    """[3, 4] float32 M = [R | t] with x_world = R x + t: the rotation by yaw_degrees about the direction `up` through the point
    `pivot`, then the translation `position`: R by Rodrigues' formula, t = pivot - R pivot + position.  Computed in float64 on the
    host and rounded once."""
    up, position, pivot = (np.asarray(a, np.float64).reshape(-1) for a in (up, position, pivot))
    if up.shape != (3,) or position.shape != (3,) or pivot.shape != (3,) or not all(np.isfinite(a).all() for a in (up, position, pivot)):
        raise ValueError("up, position and pivot must be 3 finite numbers each")
    if not np.isfinite(float(yaw_degrees)):
        raise ValueError(f"yaw_degrees={yaw_degrees} is not finite")
    if not np.linalg.norm(up) > 0:
        raise ValueError("up has no direction")
    k = up / np.linalg.norm(up)
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    a = np.radians(float(yaw_degrees))
    R = np.eye(3) + np.sin(a) * Kx + (1.0 - np.cos(a)) * (Kx @ Kx)
    M = np.concatenate([R, (pivot - R @ pivot + position)[:, None]], 1)
    return torch.from_numpy(M.astype(np.float32)).to(device or "cpu")


def check_rigid(M, name: str = "placement") -> np.ndarray:
    """M as float64 [3, 4] or [N, 3, 4], or a ValueError: finite, |R R^T - I| <= RIGID_TOLERANCE in every entry, det R > 0."""
    try:
        m = np.asarray(M.detach().cpu().numpy() if torch.is_tensor(M) else M, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be None or an array [3, 4] or [N, 3, 4] (got {type(M).__name__})") from None
    if m.shape[-2:] != (3, 4) or m.ndim not in (2, 3):
        raise ValueError(f"{name} must be None or an array [3, 4] or [N, 3, 4] (got {list(m.shape)})")
    if not np.isfinite(m).all():
        raise ValueError(f"{name} is not finite")
    R = m[..., :3]
    off = float(np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max()) if m.size else 0.0
    if off > RIGID_TOLERANCE or (m.size and float(np.linalg.det(R).min()) <= 0):
        raise ValueError(f"{name} is not rigid: |R R^T - I| = {off:.3g} (at most {RIGID_TOLERANCE:g}) and det R must be positive")
    return m


def camera_in_body_frame(camera_pos, M):
    """camera_pos [., 3] as body coordinates of a body placed by M ([3, 4] or [N, 3, 4], x_world = R x + t): R^T (c - t) with d = c -
    t as (d0 R[0] + d1 R[1]) + d2 R[2], float32 elementwise torch ops on the device of camera_pos (no library matrix product: the
    bits do not depend on the batch); [1, 3] for a shared placement and camera, else [N, 3]."""
    M = M.reshape(-1, 3, 4)
    d = camera_pos.reshape(-1, 3) - M[:, :, 3]
    return ((d[:, 0:1] * M[:, 0, :3] + d[:, 1:2] * M[:, 1, :3]) + d[:, 2:3] * M[:, 2, :3]).contiguous()


def _as_rasterizer(body, p: int, height: int, width: int, near: float) -> BodyRasterizer:
    flip = None
    if isinstance(body, dict):
        if "body" not in body or set(body) - {"body", "flip_uv"}:
            raise TypeError(f"bodies[{p}]: a dict holds `body` and optionally `flip_uv` (got keys {sorted(body)})")
        body, flip = body["body"], bool(body.get("flip_uv", False))
    elif isinstance(body, (tuple, list)) and len(body) == 2 and isinstance(body[1], (bool, np.bool_)):
        body, flip = body[0], bool(body[1])
    if isinstance(body, BodyRasterizer):
        rz = copy.copy(body)                                                  # shallow: the validated tables (and device copies) are shared
        rz.height, rz.width, rz.near = height, width, near
        if flip is not None:
            rz.flip_uv = flip
        return rz
    if not isinstance(body, BodySurface) and not (isinstance(body, (tuple, list)) and len(body) in (3, 4)):
        raise TypeError(f"bodies[{p}] must be a BodySurface, a BodyRasterizer or a tuple (vi, vt, vti[, n_verts]), optionally paired with "
                        f"flip_uv (got {type(body).__name__})")
    return BodyRasterizer(body if isinstance(body, BodySurface) else tuple(body), height, width, bool(flip), near)


class SceneRasterizer(RenderArguments):
    """1 to 4 triangle meshes with UV layouts and one image size, ready to rasterise together.  Each entry of `bodies` is a
    BodySurface (whose validated topology tables are shared, not copied), a BodyRasterizer (its tables and flip_uv) or a tuple (vi
    [F, 3], vt [T, 2], vti [F, 3][, n_verts]); `(entry, flip_uv)` or {"body": entry, "flip_uv": bool} sets the body's flip.  The
    merged face table -- every body's vi with the earlier bodies' vertex counts added -- is built here, once.  A face with a corner
    nearer than `near` along the camera's z axis is dropped whole: one near plane for all bodies."""

    def __init__(self, bodies, height: int, width: int, near: float = 1e-3):
        if isinstance(bodies, (BodySurface, BodyRasterizer)) or not isinstance(bodies, (tuple, list)):
            raise TypeError("SceneRasterizer takes a sequence of bodies")
        if not 1 <= len(bodies) <= MAX_BODIES:
            raise ValueError(f"a scene holds 1 to {MAX_BODIES} bodies (got {len(bodies)})")
        self.height, self.width, self.near = int(height), int(width), float(near)
        self.bodies = [_as_rasterizer(b, p, self.height, self.width, self.near) for p, b in enumerate(bodies)]
        self.P = len(self.bodies)
        self.V = [b.V for b in self.bodies]
        self.F = [b.F for b in self.bodies]
        self.sum_V, self.sum_F = sum(self.V), sum(self.F)
        if 3 * self.sum_F >= 1 << 31 or 3 * self.sum_V >= 1 << 31:
            raise ValueError(f"the bodies hold {self.sum_V} vertices and {self.sum_F} faces together: need 3 sum V, 3 sum F < 2^31")
        starts = np.concatenate([[0], np.cumsum(self.V)])
        host = lambda b: b.surface.vi if b.surface is not None else b._vi
        self.faces = np.ascontiguousarray(np.concatenate([host(b) + starts[p] for p, b in enumerate(self.bodies)]), np.int32)
        self._faces_dev = {}

    def _faces(self, device):
        key = str(device)
        if key not in self._faces_dev:
            self._faces_dev[key] = torch.from_numpy(self.faces).to(device)
        return self._faces_dev[key]

    def _sequence(self, x, name: str):
        if not isinstance(x, (tuple, list)) or len(x) != self.P:
            got = f"{len(x)} entries" if isinstance(x, (tuple, list)) else type(x).__name__
            raise A2PError(f"{name} must be a sequence of {self.P} entries, one per body (got {got})")
        return list(x)

    def scratch_bytes_per_frame(self, supersample: int) -> int:
        """proj and key of one frame: 12 sum V + 8 S^2 H W."""
        return self._scratch_bytes(self.sum_V, supersample)

    def render(self, verts, textures, K, Rt, placements=None, supersample: int = 1, background=None, max_bytes: int = 1 << 30) -> dict:
        """{"render": [N, C, H, W], "alpha": [N, 1, H, W], "depth": [N, 1, H, W], "body_alpha": [N, P, H, W]} of the bodies seen
        together.  verts: P tensors [N, V_p, 3]; textures: P tensors [N or 1, C, Ht_p, Wt_p] with one C (1 to 16) and sizes of
        their own; placements: None, or P entries None / [3, 4] / [N, 3, 4] (x_world = R x + t; None: the vertices are world
        coordinates already); K [N or 1, 3, 3], Rt [N or 1, 3, 4].  supersample x supersample samples per pixel (1 to 4; 1 is the
        plain render).  alpha is the covered fraction of the pixel's samples, body_alpha[p] body p's share of them (their sum is
        alpha), render the mean over all samples of each sample's nearest body's texture (premultiplied), depth the same mean of
        the samples' camera-space depths.  background as in BodyRasterizer.render_antialiased: a fully covered pixel does not read
        it, an uncovered one holds its value itself, the others render + (1 - alpha) background.  Frames are processed in chunks
        whose scratch (12 sum V + 8 S^2 H W bytes a frame) stays below max_bytes; a frame's bits do not depend on the chunking."""
        s = self._supersample(supersample)
        if int(max_bytes) < 1:
            raise A2PError(f"max_bytes={max_bytes}: need a positive byte budget")
        verts, textures = self._sequence(verts, "verts"), self._sequence(textures, "textures")
        placements = [None] * self.P if placements is None else self._sequence(placements, "placements")
        N = verts[0].shape[0] if torch.is_tensor(verts[0]) and verts[0].dim() == 3 else None
        for p in range(self.P):
            verts[p] = self._verts(verts[p], self.V[p], f"verts[{p}]", N)
        N, dev = verts[0].shape[0], verts[0].device
        C = textures[0].shape[1] if torch.is_tensor(textures[0]) and textures[0].dim() == 4 else None
        tex_per, place_per = [0] * self.P, [0] * self.P
        for p in range(self.P):
            if verts[p].device != dev:
                raise A2PError(f"verts[{p}] is on {verts[p].device}, verts[0] on {dev}")
            textures[p], tex_per[p] = self._tex(textures[p], N, dev, f"textures[{p}]", C, planes_below_2_31=True)    # C is None: textures[0] is refused
            if placements[p] is not None:
                placements[p], place_per[p] = self._camera(placements[p], f"placements[{p}]", 4, N, dev)
        K, k_per = self._camera(K, "K", 3, N, dev)
        Rt, rt_per = self._camera(Rt, "Rt", 4, N, dev)
        bg, bg_per = self._background(background, C, verts[0])
        H, W, P = self.height, self.width, self.P
        new = lambda c: torch.empty(N, c, H, W, dtype=torch.float32, device=dev)
        out = {"render": new(C), "alpha": new(1), "depth": new(1), "body_alpha": new(P)}
        if N == 0:
            return out
        tables = [b._tables(dev) for b in self.bodies]
        faces = self._faces(dev)
        lib = _lib.load()
        desc = (_lib.A2PSceneBody * P)()
        with _lib.on_device_of(verts[0]):
            for a, b, proj, key in self._chunks(N, self.sum_V, s, max_bytes, dev):
                part = lambda x, per: x[a:b] if per else x
                for p in range(P):
                    tex = part(textures[p], tex_per[p])
                    desc[p] = _lib.A2PSceneBody(
                        _lib.ptr(verts[p][a:b]), _lib.ptr(None if placements[p] is None else part(placements[p], place_per[p])), _lib.ptr(tex),
                        _lib.ptr(tables[p]["vt"]), _lib.ptr(tables[p]["vti"]), self.V[p], self.F[p], self.bodies[p].T, tex.shape[2], tex.shape[3],
                        int(self.bodies[p].flip_uv), place_per[p], tex_per[p])
                _lib.check(lib.a2p_scene_render(
                    desc, P, _lib.ptr(faces), b - a, _lib.ptr(part(K, k_per)), k_per, _lib.ptr(part(Rt, rt_per)), rt_per, H, W, s, self.near, C,
                    _lib.ptr(None if bg is None else part(bg, bg_per)), bg_per, _lib.ptr(proj), _lib.ptr(key), _lib.ptr(out["render"][a:b]),
                    _lib.ptr(out["alpha"][a:b]), _lib.ptr(out["depth"][a:b]), _lib.ptr(out["body_alpha"][a:b]), _lib.current_stream(dev)),
                    "a2p_scene_render")
        return out

# ------------------------------------------------------------------------------------------------ people
def conversation_inputs(result, repetition: int = 0):
    """(poses, face_codes, audio) of sample.conversation.generate_conversation's return value for the two functions below: per
    person the repetition's `pose` [T, .] and `face` [T, .], and audio float64 [samples, 2], channel p person p's own microphone as
    the models heard it.  A result with a person that is None (heard but not animated) is refused."""
    if not isinstance(result, dict) or not isinstance(result.get("people"), (tuple, list)) or not result["people"]:
        raise A2PError("result must be the dict generate_conversation returns (key `people`)")
    poses, codes, audio = [], [], []
    for p, person in enumerate(result["people"]):
        if person is None:
            raise A2PError(f"people[{p}] is None: this person was heard but not animated, so there is nothing to render")
        for key in ("pose", "face", "audio"):
            if key not in person:
                raise A2PError(f"people[{p}] holds no `{key}` (keys: {sorted(person)})")
        pose, face, own = np.asarray(person["pose"]), np.asarray(person["face"]), np.asarray(person["audio"])
        if pose.ndim != 3 or face.ndim != 3 or pose.shape[:2] != face.shape[:2]:
            raise A2PError(f"people[{p}]: `pose` must be [R, T, .] and `face` [R, T, .] with the same R and T (got {list(pose.shape)} and "
                           f"{list(face.shape)})")
        if not 0 <= int(repetition) < pose.shape[0]:
            raise A2PError(f"repetition={repetition}: people[{p}] holds {pose.shape[0]} repetitions")
        if own.ndim != 2 or own.shape[0] != 2:
            raise A2PError(f"people[{p}]: `audio` must be [2, samples] (own, partner) (got {list(own.shape)})")
        poses.append(pose[int(repetition)])
        codes.append(face[int(repetition)])
        audio.append(own[0].astype(np.float64))
    if len({len(a) for a in audio}) != 1 or len({x.shape[0] for x in poses}) != 1:
        raise A2PError("the people of a conversation have the same number of frames and samples")
    return poses, codes, np.stack(audio, 1)


def _people(avatars, poses, face_codes, placements):
    if not isinstance(avatars, (tuple, list)) or not 1 <= len(avatars) <= MAX_BODIES or not all(isinstance(a, Avatar) for a in avatars):
        raise A2PError(f"avatars must be a sequence of 1 to {MAX_BODIES} Avatar tuples")
    P = len(avatars)
    for name, x in (("poses", poses), ("face_codes", face_codes), ("placements", placements)):
        if not isinstance(x, (tuple, list)) or len(x) != P:
            got = f"{len(x)} entries" if isinstance(x, (tuple, list)) else type(x).__name__
            raise A2PError(f"{name} must be a sequence of {P} entries, one per avatar (got {got})")
    return P


def render_conversation_motion(avatars, poses, face_codes, placements, K, Rt, height: int, width: int, camera_pos=None,
                               body_embs: str = "per_frame", max_bytes: int = 1 << 30, supersample: int = 1, background=None):
    """uint8 frames [T, H, C W, 3] (or [B, T, H, C W, 3]) on the GPU of P people in one world seen by C cameras side by side:
    encoder.render_codes_motion for a conversation.  avatars: P Avatar tuples; poses and face_codes: P sequences of sampler output
    on the same leading axes (conversation_inputs gives them); placements: P host arrays [3, 4] or [T.., 3, 4] (x_world = R x + t,
    what `placement` returns) or None; each is checked rigid on the host (|R R^T - I| <= 1e-4, det R > 0) before any GPU work and
    uploaded once; None skips the transform entirely.  K [C, 3, 3], Rt [C, 3, 4]; camera_pos [C, 3] (world) defaults to
    render.camera_centre(Rt).

    Per chunk of frames every person is encoded, decoded and posed in their own frame with their own networks; per camera the
    view-dependent texture gets the camera position in that body's frame, R^T (c - t) (float32 on the GPU; c itself without a
    placement), then one SceneRasterizer.render shows all of them, composited in linear light by the rules of
    texture.display_frames: background (a display colour or [H, W, 3] / [3, H, W] panel in [0, 255]) is converted by
    display_to_linear, the image passed through linear_to_display, and a pixel no sample covers holds the background's bytes
    exactly.  A chunk's activations (all people's) stay under max_bytes, at least one frame; a frame's result does not depend on
    the chunking."""
    from . import encoder as E
    from .texture import display_background, linear_to_display
    P = _people(avatars, poses, face_codes, placements)
    H, W = int(height), int(width)
    avatar.check_body_embs(body_embs)
    leads = [tuple(torch.as_tensor(x).shape[:-1]) for x in face_codes]           # each person's poses are held against these below
    if len(set(leads)) != 1:
        raise A2PError(f"the people of a conversation share their frames: face_codes have leading axes {[list(ld) for ld in leads]}")
    host_place = [None if m is None else check_rigid(m, f"placements[{p}]") for p, m in enumerate(placements)]
    shown, linear = display_background(background, H, W)
    scene = SceneRasterizer([a.surface for a in avatars], H, W)
    s = scene._supersample(supersample)
    frames, codes, lead = [], [], None
    for p, a in enumerate(avatars):
        avatar.check_pose_width(a.skeleton, a.decoder, f"avatars[{p}]: ")
        avatar.check_embedding_widths(a.body_encoder, a.face_encoder, a.decoder, f"avatars[{p}]: ")
        if a.surface.V != a.skeleton.V:
            raise A2PError(f"avatars[{p}]: the skeleton skins V={a.skeleton.V} vertices; the surface has V={a.surface.V}")
        f, c, ld = E.clip_inputs("render_conversation_motion", a.skeleton, a.face_decoder, a.face_encoder, a.body_encoder, poses[p], face_codes[p])
        if lead is not None and tuple(ld) != tuple(lead):
            raise A2PError(f"the people of a conversation share their frames: person 0 has {list(lead)}, person {p} {list(ld)}")
        lead = ld
        frames.append(f), codes.append(c)
    N, dev = frames[0].shape[0], frames[0].device
    for p, m in enumerate(host_place):
        if m is not None and m.ndim == 3 and m.shape[0] not in (1, N):
            raise A2PError(f"placements[{p}] must be [3, 4] or [{N} or 1, 3, 4] (got {list(m.shape)})")
    K, Rt, camera_pos, C = avatar.cameras(K, Rt, camera_pos, dev)
    place = [None if m is None else torch.from_numpy(np.ascontiguousarray(m.reshape(-1, 3, 4), np.float32)).to(dev) for m in host_place]
    per_frame = sum(E.activation_bytes_per_frame(a.face_decoder, a.face_encoder, a.body_encoder, a.skeleton)
                    + a.decoder.activation_bytes_per_frame() + a.texture.activation_bytes_per_frame() for a in avatars)
    shown, linear = (None if x is None else x.to(dev) for x in (shown, linear))
    out = torch.empty(N, H, C * W, 3, dtype=torch.uint8, device=dev)
    rest = [E.rest_embs(a.body_encoder, a.skeleton, dev) if body_embs == "rest" and N else None for a in avatars]
    for lo, hi in avatar.frame_chunks(N, max_bytes, per_frame):
        verts, preds, here = [], [], []
        for p, a in enumerate(avatars):
            embs, face_embs = E.encode_chunk(a.face_decoder, a.face_encoder, a.body_encoder, a.skeleton, frames[p][lo:hi], codes[p][lo:hi],
                                              None, rest[p])
            pr, posed = avatar.decode_and_pose(a.decoder, a.skeleton, frames[p][lo:hi], embs.contiguous(), face_embs)
            verts.append(posed), preds.append(pr)
            here.append(None if place[p] is None else (place[p][lo:hi] if place[p].shape[0] == N and N != 1 else place[p][0]))
        for c in range(C):
            tex = []
            for p, a in enumerate(avatars):
                cam = camera_pos[c:c + 1] if here[p] is None else camera_in_body_frame(camera_pos[c:c + 1], here[p])
                tex.append(a.texture.forward(verts[p], preds[p]["tex_mean_rec"], cam,
                                             motion=frames[p][lo:hi] if a.texture.pose_shadow is not None else None)["tex_rec"])
            got = scene.render(verts, tex, K[c:c + 1], Rt[c:c + 1], here, s, linear, max_bytes)
            image = linear_to_display(got["render"])
            if shown is not None:
                image = torch.where(got["alpha"] == 0, shown, image)
            out[lo:hi, :, c * W:(c + 1) * W] = avatar.uint8_panel(image)
    return out.reshape(*lead, H, C * W, 3)


def render_conversation_video(avatars, poses, face_codes, placements, K, Rt, height: int, width: int, path, audio=None, audio_rate=None,
                              fps=30, quality: int = 90, subsampling: str = "420", slice_frames: int = 32, **kw) -> int:
    """render_conversation_motion over slices of slice_frames frames of the time axis, every slice encoded and appended to the AVI
    file `path` before the next is rendered, as video.render_codes_video does for one person.  poses[p] [T, .] and face_codes[p]
    [T, .]: one sequence per person; placements [3, 4] or [T, 3, 4]; audio ([samples] or [samples, channels], e.g. one channel per
    person from conversation_inputs) is written as it is; **kw goes to render_conversation_motion (camera_pos, body_embs,
    max_bytes, supersample, background).  A frame's bytes do not depend on the slicing.  Returns the number of frames."""
    from .video import MJPEGWriter
    P = _people(avatars, poses, face_codes, placements)
    poses, face_codes = [torch.as_tensor(x) for x in poses], [torch.as_tensor(x) for x in face_codes]
    T = poses[0].shape[0] if poses[0].dim() == 2 else None
    for p in range(P):
        if poses[p].dim() != 2 or face_codes[p].dim() != 2 or poses[p].shape[0] != T or face_codes[p].shape[0] != T:
            raise A2PError(f"poses and face_codes must be [T, .] per person with one T (person {p}: {list(poses[p].shape)} and "
                           f"{list(face_codes[p].shape)}; T = {T})")
    host_place = [None if m is None else check_rigid(m, f"placements[{p}]") for p, m in enumerate(placements)]
    for p, m in enumerate(host_place):
        if m is not None and m.ndim == 3 and m.shape[0] not in (1, T):
            raise A2PError(f"placements[{p}] must be [3, 4] or [{T} or 1, 3, 4] (got {list(m.shape)})")
    C = torch.as_tensor(K).shape[0]
    step = max(1, int(slice_frames))
    with MJPEGWriter(path, int(height), C * int(width), fps, quality, subsampling, audio, audio_rate) as w:
        for a in range(0, T, step):
            part = [None if m is None else (m[a:a + step] if m.ndim == 3 and m.shape[0] == T and T != 1 else m) for m in host_place]
            w.write(render_conversation_motion(avatars, [x[a:a + step] for x in poses], [x[a:a + step] for x in face_codes], part, K, Rt,
                                               height, width, **kw))
    return int(T)


# ------------------------------------------------------------------------------------------------ command line
def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m audio2photoreal_amd.scene",
                                 description="Video frames of several people in one scene: per person a results.npy, assets and a checkpoint.")
    ap.add_argument("--results", required=True, nargs="+", help="per person a results.npy: a pickled dict with `pose` [R, T, 104] and `face` "
                    "[R, T, 256], un-normalised")
    ap.add_argument("--assets", required=True, nargs="+", help="per person a static_assets.pt")
    ap.add_argument("--checkpoint", required=True, nargs="+", help="per person the body model's state dict")
    ap.add_argument("--yaw", type=float, nargs="+", default=None, help="per person the rotation about --up in degrees (default 0)")
    ap.add_argument("--position", type=float, nargs="+", default=None, help="per person x y z: the translation after the rotation (default 0 0 0)")
    ap.add_argument("--pivot", type=float, nargs="+", default=None, help="per person x y z: the point the rotation goes through (default 0 0 0)")
    ap.add_argument("--repetition", type=int, default=0, help="which of the R sequences of every results.npy")
    ap.add_argument("--out", required=True, help="frames.npy: a uint8 array [T, H, C W, 3]")
    avatar.add_camera_arguments(ap, per="camera", eye_help="in front of the first frame's bounding box along +z, far enough to see everyone")
    avatar.add_render_arguments(ap)
    avatar.add_video_arguments(ap)
    avatar.add_network_arguments(ap, encoders=True)
    return ap


def main(argv=None) -> int:
    from . import render as R
    args = parser().parse_args(argv)
    P = len(args.results)
    if not 1 <= P <= MAX_BODIES or len(args.assets) != P or len(args.checkpoint) != P:
        raise A2PError(f"--results, --assets and --checkpoint take one file per person, 1 to {MAX_BODIES} people (got {P}, {len(args.assets)} "
                       f"and {len(args.checkpoint)})")
    yaw = [0.0] * P if args.yaw is None else list(args.yaw)
    position = [0.0] * (3 * P) if args.position is None else list(args.position)
    pivot = [0.0] * (3 * P) if args.pivot is None else list(args.pivot)
    if len(yaw) != P or len(position) != 3 * P or len(pivot) != 3 * P:
        raise A2PError(f"--yaw takes {P} numbers, --position and --pivot {3 * P} (x y z per person)")
    if args.audio is not None and args.video is None:
        raise A2PError("--audio goes with --video")
    poses, faces = [], []
    for path in args.results:
        pose, face = avatar.load_codes_clip(path)
        if pose.ndim != 3 or face.ndim != 3 or pose.shape[:2] != face.shape[:2] or not 0 <= args.repetition < pose.shape[0]:
            raise A2PError(f"{path}: `pose` must be [R, T, P] and `face` [R, T, F] with the same R > {args.repetition} and T (got "
                           f"{list(pose.shape)} and {list(face.shape)})")
        window = avatar.frame_window(args.frames)
        poses.append(pose[args.repetition][window]), faces.append(face[args.repetition][window])
    if len({len(x) for x in poses}) != 1:
        raise A2PError(f"the people have {[len(x) for x in poses]} frames: need the same number")
    avatar.require_gpu("the frames are rendered")
    avatars = [load_avatar(a, c, args) for a, c in zip(args.assets, args.checkpoint)]
    places = [placement(yaw[p], position[3 * p:3 * p + 3], args.up, pivot[3 * p:3 * p + 3]).numpy() for p in range(P)]
    H, W = args.size
    poses_gpu = [torch.from_numpy(x).to("cuda") for x in poses]
    first = [a.skeleton.pose_vertices(x[:1]).cpu().numpy().astype(np.float64)[0] @ m[:, :3].T.astype(np.float64) + m[:, 3]
             for a, x, m in zip(avatars, poses_gpu, places)]                    # frames the default camera: everyone's first frame, placed
    K, Rt = R._camera_from_args(args, np.concatenate(first)[None], H, W)
    kw = dict(body_embs=args.body_embs, max_bytes=args.max_bytes, supersample=args.supersample, background=args.background)
    frames = render_conversation_motion(avatars, poses_gpu, faces, places, K, Rt, H, W, **kw).cpu().numpy()
    np.save(args.out, frames)
    print(f"{args.out}: frames {list(frames.shape)} uint8, {P} people")
    if args.video is not None:
        audio, rate = avatar.video_audio(args)
        render_conversation_video(avatars, poses_gpu, faces, places, K, Rt, H, W, args.video, audio=audio, audio_rate=rate, fps=args.fps, **kw)
        print(f"{args.video}: {frames.shape[0]} frames at {args.fps:g} fps")
    return 0


if __name__ == "__main__":
    sys.exit(main())
