"""Rendered images of the posed body mesh on the MI355X: z-buffer rasterisation, perspective-correct attribute images and UV
texture sampling -- the third stage of the reference's renderer (visualize/ca_body/utils/render.py: RenderLayer, which gets them
from pytorch3d's MeshRasterizer and TexturesUV.sample_textures), as HIP launches for all frames (csrc/kernels_render.h), and
anti-aliased images over a background, which the reference does not have (csrc/kernels_render_aa.h).

    python -m audio2photoreal_amd.render --geometry geometry.npy --assets static_assets.pt --out frames.npy [--size H W]
                                         [--camera-json FILE | --eye x y z --target x y z --fov deg] [--outputs depth normals ...]
                                         [--frames A:B] [--png-dir DIR] [--supersample S]

`BodyRasterizer` is built once from a `BodySurface` (whose validated topology tables it shares), from arrays (`from_arrays`) or
from the topology the reference reads (`from_static_assets`).  Cameras are OpenCV pinholes: K [N or 1, 3, 3], Rt [N or 1, 3, 4],
x right, y down, z forward; pixel (row i, column j) has centre (j + 0.5, i + 0.5).  The methods take float32 tensors that live on
the GPU and run on the caller's current stream; there is no CPU path.  INTEGRATION.md "Rendered images" states every rule."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

from . import _lib, avatar
from ._lib import A2PError
from .surface import BodySurface, index_array

OUTPUTS = {"depth": 1, "normals": 3, "view_cos": 1, "positions": 3, "mask": 1}     # render_motion's images and their channels


def look_at(eye, target, up, height: int, width: int, fov_degrees: float, device=None):
    """(K [3, 3], Rt [3, 4]) float32 of a pinhole camera at `eye` looking at `target`, in the OpenCV convention (x right, y down,
    z forward): the rows of R are the camera axes in world coordinates, t = -R eye.  `up` is the world direction that points up
    in the image; fov_degrees is the vertical field of view; the principal point is the image centre (width / 2, height / 2)."""
    eye, target, up = (np.asarray(a, np.float64).reshape(-1) for a in (eye, target, up))
    if eye.shape != (3,) or target.shape != (3,) or up.shape != (3,) or not all(np.isfinite(a).all() for a in (eye, target, up)):
        raise ValueError("eye, target and up must be 3 finite numbers each")
    if int(height) < 1 or int(width) < 1:
        raise ValueError(f"a {height} x {width} image: need height, width >= 1")
    if not 0.0 < float(fov_degrees) < 180.0:
        raise ValueError(f"fov_degrees={fov_degrees} is outside (0, 180)")
    z = target - eye
    if not np.linalg.norm(z) > 0:
        raise ValueError("eye and target coincide: the camera has no direction")
    z = z / np.linalg.norm(z)
    x = np.cross(z, up)
    if not np.linalg.norm(x) > 1e-9 * max(np.linalg.norm(up), 1e-300):
        raise ValueError("up is parallel to the viewing direction")
    x = x / np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    f = 0.5 * int(height) / np.tan(np.radians(float(fov_degrees)) / 2)
    K = np.array([[f, 0.0, int(width) / 2], [0.0, f, int(height) / 2], [0.0, 0.0, 1.0]])
    Rt = np.concatenate([R, (-R @ eye)[:, None]], 1)
    return torch.from_numpy(K.astype(np.float32)).to(device or "cpu"), torch.from_numpy(Rt.astype(np.float32)).to(device or "cpu")


class RenderArguments:
    """The argument checks and the chunking that BodyRasterizer and scene.SceneRasterizer share; both have a height and a width."""

    _tensor = staticmethod(BodySurface._tensor)

    def _verts(self, verts, V: int, name: str = "verts", N=None):
        return self._tensor(verts, name, f"[{'N' if N is None else N}, {V}, 3]", lambda s: len(s) == 3 and s[1:] == (V, 3) and N in (None, s[0]))

    def _tex(self, tex, N: int, dev, name: str = "tex", C=None, beside: str = "verts", planes_below_2_31: bool = False):
        """A texture as (contiguous tensor, per-frame flag): [N or 1, C, Ht, Wt] on dev, with C channels when C is given."""
        C_max = _lib.RENDER_MAX_CHANNELS
        tex = self._tensor(tex, name, f"[{N} or 1, {'C' if C is None else C}, Ht, Wt] with 1 <= C <= {C_max}",
                           lambda s: len(s) == 4 and s[0] in (1, N) and 1 <= s[1] <= C_max and C in (None, s[1]) and min(s[2:]) >= 1
                           and (not planes_below_2_31 or s[2] * s[3] < 1 << 31))
        if tex.device != dev:
            raise A2PError(f"{name} is on {tex.device}, {beside} on {dev}")
        return tex, int(tex.shape[0] == N and N != 1)

    def _camera(self, x, name: str, cols: int, N: int, dev):
        """A camera array as (contiguous tensor, per-frame flag): [N or 1, 3, cols], or [3, cols] for one shared by all frames."""
        x = self._tensor(x, name, f"[{N} or 1, 3, {cols}]",
                         lambda s: s == (3, cols) or (len(s) == 3 and s[1:] == (3, cols) and s[0] in (1, N)))
        if x.device != dev:
            raise A2PError(f"{name} is on {x.device}, verts on {dev}")
        return x, int(x.dim() == 3 and x.shape[0] == N and N != 1)

    def _supersample(self, supersample) -> int:
        s = int(supersample)
        if s != supersample or not 1 <= s <= _lib.RENDER_MAX_SUPERSAMPLE:
            raise ValueError(f"supersample={supersample} is outside [1, {_lib.RENDER_MAX_SUPERSAMPLE}] samples per axis")
        for name, size in (("height", self.height), ("width", self.width)):
            if s * size > _lib.RENDER_MAX_SIZE:
                raise ValueError(f"supersample={s} x {name}={size} exceeds {_lib.RENDER_MAX_SIZE} samples per axis")
        return s

    def _background(self, background, C, verts):
        """A background as (contiguous [n, C, H, W] tensor or None, per-frame flag): None, a colour [C] or [N or 1, C, H, W] on the
        device of verts.  Checked before anything is asked of the GPU."""
        if background is None or C is None:                                   # C is None: tex is malformed and is refused next
            return None, 0
        H, W = self.height, self.width
        N = verts.shape[0] if torch.is_tensor(verts) and verts.dim() else 1
        if not torch.is_tensor(background):
            raise A2PError(f"background must be None or a tensor on the MI355X (got {type(background).__name__})")
        shape = tuple(background.shape)
        if background.dtype != torch.float32 or not (shape == (C,) or (len(shape) == 4 and shape[1:] == (C, H, W) and shape[0] in (1, N))):
            raise A2PError(f"background must be float32 [{C}] or [{N} or 1, {C}, {H}, {W}] (got {background.dtype} {list(shape)})")
        if torch.is_tensor(verts) and background.device != verts.device:
            raise A2PError(f"background is on {background.device}, verts on {verts.device}")
        bg = background.reshape(1, C, 1, 1).expand(1, C, H, W) if background.dim() == 1 else background
        return bg.contiguous(), int(bg.shape[0] == N and N != 1)

    def _scratch_bytes(self, V: int, s: int) -> int:
        return 12 * V + 8 * s * s * self.height * self.width                  # proj and key of one frame

    def _chunks(self, N: int, V: int, s: int, max_bytes, dev):
        """(a, b, proj, key): frames a..b-1 per chunk; its scratch proj [., V, 3] and key [., s H, s W] stays below max_bytes (or is one frame)."""
        step = min(N, max(1, int(max_bytes) // self._scratch_bytes(V, s)))
        proj = torch.empty(step, V, 3, dtype=torch.float32, device=dev)
        key = torch.empty(step, s * self.height, s * self.width, dtype=torch.int64, device=dev)
        for a in range(0, N, step):
            yield a, min(N, a + step), proj, key


class BodyRasterizer(RenderArguments):
    """A triangle mesh with a UV layout and an image size, ready to rasterise.  `surface_or_arrays` is a BodySurface or a tuple
    (vi [F, 3], vt [T, 2], vti [F, 3]) or (vi, vt, vti, n_verts).  flip_uv samples textures at v <- 1 - v (the meaning it has in BodySurface); a face with
    a corner nearer than `near` along the camera's z axis is dropped whole."""

    def __init__(self, surface_or_arrays, height: int, width: int, flip_uv: bool = False, near: float = 1e-3):
        if isinstance(surface_or_arrays, BodySurface):
            self.surface = surface_or_arrays
            self.V, self.F, self.T = self.surface.V, self.surface.F, self.surface.T
        else:
            try:
                vi, vt, vti, n_verts = (*surface_or_arrays, None)[:4]
            except (TypeError, ValueError):
                raise TypeError("BodyRasterizer takes a BodySurface or a tuple (vi, vt, vti)") from None
            self.surface = None
            self._set_arrays(vi, vt, vti, n_verts)
        self.height, self.width = int(height), int(width)
        for name, size in (("height", self.height), ("width", self.width)):
            if not 1 <= size <= _lib.RENDER_MAX_SIZE:
                raise ValueError(f"{name}={size} is outside [1, {_lib.RENDER_MAX_SIZE}]")
        self.near = float(near)
        if not (0.0 < self.near < float("inf")):
            raise ValueError(f"near={near} must be a positive finite distance")
        self.flip_uv = bool(flip_uv)
        self._dev = {}

    def _set_arrays(self, vi, vt, vti, n_verts):
        vt_np = np.asarray(vt.detach().cpu().numpy() if torch.is_tensor(vt) else vt)
        if vt_np.ndim != 2 or vt_np.shape[1] != 2 or vt_np.shape[0] < 1:
            raise ValueError(f"vt must be [T >= 1, 2] (got {list(vt_np.shape)})")
        self._vt = np.ascontiguousarray(vt_np, np.float32)
        bad = np.argwhere(~np.isfinite(self._vt))
        if bad.size:
            raise ValueError(f"vt{list(map(int, bad[0]))} is not finite ({self._vt[tuple(bad[0])]})")
        raw_vi = np.asarray(vi.detach().cpu().numpy() if torch.is_tensor(vi) else vi)
        V = int(n_verts) if n_verts is not None else int(raw_vi.max(initial=-1)) + 1
        if V < 1:
            raise ValueError(f"the mesh has V={V} vertices; need at least 1")
        self._vi = index_array("vi", raw_vi, 3, V, "V")
        self._vti = index_array("vti", vti, 3, self._vt.shape[0], "T")
        if self._vi.shape[0] < 1 or self._vti.shape[0] != self._vi.shape[0]:
            raise ValueError(f"vi holds F={self._vi.shape[0]} faces and vti {self._vti.shape[0]}; need the same F >= 1")
        self.V, self.F, self.T = V, self._vi.shape[0], self._vt.shape[0]

    @classmethod
    def from_arrays(cls, vi, vt, vti, height: int, width: int, n_verts=None, flip_uv: bool = False, near: float = 1e-3):
        """vi [F, 3] vertex indices; vt [T, 2] texture coordinates; vti [F, 3] texture indices.  V is n_verts, else the largest
        index + 1.  Unlike BodySurface this asks nothing of the vertex-to-texture table: a vertex may be unused."""
        return cls((vi, vt, vti, n_verts), height, width, flip_uv, near)

    @classmethod
    def from_static_assets(cls, assets, height: int, width: int, flip_uv: bool = False, near: float = 1e-3):
        """The mapping the reference's AutoEncoder.__init__ reads: assets["topology"] with vi, vt, vti and v2uv."""
        return cls(BodySurface.from_static_assets(assets), height, width, flip_uv, near)

    # -------------------------------------------------------------------------------------------- device side
    def _tables(self, device):
        if self.surface is not None:
            return self.surface._tables(device)
        key = str(device)
        if key not in self._dev:
            i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(device)
            self._dev[key] = {"vi": i32(self._vi), "vti": i32(self._vti), "vt": torch.from_numpy(self._vt).to(device)}
        return self._dev[key]

    def _fragments(self, fragments, N=None):
        if not isinstance(fragments, dict) or "face" not in fragments or "bary" not in fragments:
            raise A2PError("fragments must be the dict rasterize returns (keys face, bary)")
        face, H, W = fragments["face"], self.height, self.width
        if not torch.is_tensor(face):
            raise A2PError(f"fragments['face'] must be a tensor on the MI355X (got {type(face).__name__})")
        _lib.require_gpu_tensor(face, "fragments['face']")
        if face.dtype != torch.int32 or face.dim() != 3 or tuple(face.shape[1:]) != (H, W) or (N is not None and face.shape[0] != N):
            raise A2PError(f"fragments['face'] must be int32 [{'N' if N is None else N}, {H}, {W}] (got {face.dtype} {list(face.shape)})")
        n = face.shape[0]
        bary = self._tensor(fragments["bary"], "fragments['bary']", f"[{n}, {H}, {W}, 3]", lambda s: s == (n, H, W, 3))
        if bary.device != face.device:
            raise A2PError(f"fragments['bary'] is on {bary.device}, fragments['face'] on {face.device}")
        return face.contiguous(), bary

    def rasterize(self, verts, K, Rt) -> dict:
        """{"face": int32 [N, H, W] (-1: background), "bary": float32 [N, H, W, 3] perspective-correct barycentrics (0), "depth":
        float32 [N, H, W] camera-space z of the visible surface (0)} of verts [N, V, 3] seen through K and Rt."""
        verts = self._verts(verts, self.V)
        N, dev, H, W = verts.shape[0], verts.device, self.height, self.width
        K, k_per = self._camera(K, "K", 3, N, dev)
        Rt, rt_per = self._camera(Rt, "Rt", 4, N, dev)
        out = {"face": torch.empty(N, H, W, dtype=torch.int32, device=dev), "bary": torch.empty(N, H, W, 3, dtype=torch.float32, device=dev),
               "depth": torch.empty(N, H, W, dtype=torch.float32, device=dev)}
        if N == 0:
            return out
        t = self._tables(dev)
        proj = torch.empty(N, self.V, 3, dtype=torch.float32, device=dev)
        key = torch.empty(N, H, W, dtype=torch.int64, device=dev)
        with _lib.on_device_of(verts):
            _lib.check(_lib.load().a2p_render_rasterize(
                _lib.ptr(verts), N, self.V, _lib.ptr(t["vi"]), self.F, _lib.ptr(K), k_per, _lib.ptr(Rt), rt_per, H, W, self.near,
                _lib.ptr(proj), _lib.ptr(key), _lib.ptr(out["face"]), _lib.ptr(out["bary"]), _lib.ptr(out["depth"]),
                _lib.current_stream(dev)), "a2p_render_rasterize")
        return out

    def interpolate(self, fragments: dict, values):
        """[N, C, H, W]: values [N, V, C] (1 <= C <= 16) of the visible face's corners weighted by the pixel's barycentrics; 0 on
        background.  For normals, positions, the view cosine."""
        C_max = _lib.RENDER_MAX_CHANNELS
        values = self._tensor(values, "values", f"[N, {self.V}, C] with 1 <= C <= {C_max}",
                              lambda s: len(s) == 3 and s[1] == self.V and 1 <= s[2] <= C_max)
        N, C, dev, H, W = values.shape[0], values.shape[2], values.device, self.height, self.width
        face, bary = self._fragments(fragments, N)
        if face.device != dev:
            raise A2PError(f"fragments are on {face.device}, values on {dev}")
        out = torch.empty(N, C, H, W, dtype=torch.float32, device=dev)
        if N == 0:
            return out
        t = self._tables(dev)
        with _lib.on_device_of(values):
            _lib.check(_lib.load().a2p_render_interpolate(_lib.ptr(values), N, self.V, C, _lib.ptr(t["vi"]), self.F, _lib.ptr(face),
                                                          _lib.ptr(bary), H, W, _lib.ptr(out), _lib.current_stream(dev)),
                       "a2p_render_interpolate")
        return out

    def sample_texture(self, fragments: dict, tex):
        """[N, C, H, W]: tex [N or 1, C, Ht, Wt] (1 <= C <= 16) sampled bilinearly (border padding) at each pixel's interpolated
        texture coordinate; 0 on background."""
        face, bary = self._fragments(fragments)
        N, dev, H, W = face.shape[0], face.device, self.height, self.width
        tex, tex_per = self._tex(tex, N, dev, beside="the fragments")
        C, Ht, Wt = tex.shape[1:]
        out = torch.empty(N, C, H, W, dtype=torch.float32, device=dev)
        if N == 0:
            return out
        t = self._tables(dev)
        with _lib.on_device_of(face):
            _lib.check(_lib.load().a2p_render_texture(
                _lib.ptr(face), _lib.ptr(bary), N, H, W, _lib.ptr(t["vt"]), self.T, _lib.ptr(t["vti"]), self.F, _lib.ptr(tex),
                tex_per, C, Ht, Wt, int(self.flip_uv), _lib.ptr(out), _lib.current_stream(dev)),
                "a2p_render_texture")
        return out

    def render(self, verts, tex, K, Rt, background=None, output_filters=None) -> dict:
        """{"render": [N, C, H, W]}: RenderLayer.forward -- the texture seen through the camera, 0 on background.  background and
        output_filters are accepted only as None, like the reference's asserts."""
        if background is not None or output_filters is not None:
            raise A2PError("render: background and output_filters must be None (the reference asserts the same)")
        return {"render": self.sample_texture(self.rasterize(verts, K, Rt), tex)}

    # -------------------------------------------------------------------------------------------- anti-aliased images
    def _antialiased(self, verts, K, Rt, s: int, max_bytes, C: int, background, source, want_depth: bool):
        """What both anti-aliased methods share; source(tables, a, b) -> (export name, its arguments before the cameras, its
        arguments after `near`) for frames a..b-1.  background: what _background returned."""
        if int(max_bytes) < 1:
            raise A2PError(f"max_bytes={max_bytes}: need a positive byte budget")
        N, dev, H, W = verts.shape[0], verts.device, self.height, self.width
        K, k_per = self._camera(K, "K", 3, N, dev)
        Rt, rt_per = self._camera(Rt, "Rt", 4, N, dev)
        bg, bg_per = background
        new = lambda c: torch.empty(N, c, H, W, dtype=torch.float32, device=dev)
        out, alpha, depth = new(C), new(1), new(1) if want_depth else None
        if N == 0:
            return out, alpha, depth
        t = self._tables(dev)
        lib = _lib.load()
        with _lib.on_device_of(verts):
            for a, b, proj, key in self._chunks(N, self.V, s, max_bytes, dev):
                part = lambda x, per: x[a:b] if per else x
                name, before, after = source(t, a, b)
                _lib.check(getattr(lib, name)(
                    _lib.ptr(verts[a:b]), b - a, self.V, _lib.ptr(t["vi"]), self.F, *before, _lib.ptr(part(K, k_per)), k_per,
                    _lib.ptr(part(Rt, rt_per)), rt_per, H, W, s, self.near, *after, _lib.ptr(None if bg is None else part(bg, bg_per)),
                    bg_per, _lib.ptr(proj), _lib.ptr(key), _lib.ptr(out[a:b]), _lib.ptr(alpha[a:b]),
                    *(() if name.endswith("texture") else (_lib.ptr(None if depth is None else depth[a:b]),)),
                    _lib.current_stream(dev)), name)
        return out, alpha, depth

    def render_antialiased(self, verts, tex, K, Rt, supersample: int = 2, background=None, max_bytes: int = 1 << 30) -> dict:
        """{"render": [N, C, H, W], "alpha": [N, 1, H, W]}: the texture seen through the camera with supersample x supersample
        samples per pixel (1 to 4 per axis; INTEGRATION.md "Rendered images" states where they are).  alpha is the covered fraction
        of the pixel's samples, and render is premultiplied by it: the mean over all samples, an uncovered one counting 0.
        background (None, a colour [C] or [N or 1, C, H, W], in the texture's own linear units) is composited under it: a fully
        covered pixel does not read it, an uncovered one holds its value itself, the others render + (1 - alpha) background.
        Frames are processed in chunks whose scratch stays below max_bytes; a frame's bits do not depend on the chunking."""
        s = self._supersample(supersample)
        background = self._background(background, tex.shape[1] if torch.is_tensor(tex) and tex.dim() == 4 else None, verts)
        verts = self._verts(verts, self.V)
        N, dev = verts.shape[0], verts.device
        tex, tex_per = self._tex(tex, N, dev)
        C, Ht, Wt = tex.shape[1:]
        source = lambda t, a, b: ("a2p_render_antialiased_texture", (_lib.ptr(t["vt"]), self.T, _lib.ptr(t["vti"])),
                                  (_lib.ptr(tex[a:b] if tex_per else tex), tex_per, C, Ht, Wt, int(self.flip_uv)))
        out, alpha, _ = self._antialiased(verts, K, Rt, s, max_bytes, C, background, source, False)
        return {"render": out, "alpha": alpha}

    def interpolate_antialiased(self, verts, values, K, Rt, supersample: int = 2, max_bytes: int = 1 << 30) -> dict:
        """{"values": [N, C, H, W], "alpha": [N, 1, H, W], "depth": [N, 1, H, W]}: values [N, V, C] (1 <= C <= 16) interpolated at
        every sample and averaged like render_antialiased (premultiplied by alpha); depth is the same mean of the samples' depths."""
        s = self._supersample(supersample)
        verts = self._verts(verts, self.V)
        N, dev = verts.shape[0], verts.device
        C_max = _lib.RENDER_MAX_CHANNELS
        values = self._tensor(values, "values", f"[{N}, {self.V}, C] with 1 <= C <= {C_max}",
                              lambda s: len(s) == 3 and s[0] == N and s[1] == self.V and 1 <= s[2] <= C_max)
        if values.device != dev:
            raise A2PError(f"values are on {values.device}, verts on {dev}")
        C = values.shape[2]
        source = lambda t, a, b: ("a2p_render_antialiased_values", (), (_lib.ptr(values[a:b]), C))
        out, alpha, depth = self._antialiased(verts, K, Rt, s, max_bytes, C, (None, 0), source, True)
        return {"values": out, "alpha": alpha, "depth": depth}

    def mask(self, fragments: dict):
        """float32 [N, 1, H, W]: 1 where a face is visible, 0 on background."""
        face, _ = self._fragments(fragments)
        return (face >= 0).to(torch.float32)[:, None]


# ------------------------------------------------------------------------------------------------ convenience
def camera_centre(Rt):
    """[., 3] = -R^T t of Rt [., 3, 4] (or [3, 4]): the camera position in world coordinates."""
    Rt = Rt.reshape(-1, 3, 4)
    return -(Rt[:, :, :3].transpose(1, 2) @ Rt[:, :, 3:]).squeeze(-1).contiguous()


def render_motion(rasterizer: BodyRasterizer, surface: BodySurface, vertices, K, Rt, outputs=("depth", "normals", "view_cos"),
                  camera_pos=None, max_bytes: int = 1 << 30, supersample: int = 1) -> dict:
    """Images of posed vertices in the layouts skinning.pose_motion returns, [B, T, V, 3] or [N, V, 3] (float32 on the GPU):
    {name: [B, T, C, H, W] or [N, C, H, W]} for each name in `outputs` -- "depth" (1 channel), "normals" (3, the interpolated
    vertex normals), "view_cos" (1), "positions" (3, world coordinates) and "mask" (1).  K / Rt are [N or 1, 3, .] with N = B T;
    camera_pos ([N or 1, 3], for the view cosine) defaults to the camera centre -R^T t.

    The frames are processed in chunks whose scratch and intermediate arrays stay below max_bytes (at least one frame per chunk);
    the returned images themselves take N C H W 4 bytes per output.  A frame's result does not depend on the chunking.

    supersample = s > 1 (at most 4) anti-aliases: every output is the mean over the pixel's s x s samples of the single-sample
    image (BodyRasterizer.interpolate_antialiased), an uncovered sample counting 0.  "mask" is then the coverage, the covered
    fraction of the pixel's samples, and every other output is premultiplied by it: divide by "mask" where it is not 0 for the
    mean over the covered samples alone.  (Averaged normals are no longer unit vectors.)"""
    s = rasterizer._supersample(supersample)
    if not torch.is_tensor(vertices):
        raise A2PError(f"vertices must be a tensor on the MI355X (got {type(vertices).__name__})")
    V, H, W = rasterizer.V, rasterizer.height, rasterizer.width
    shape = tuple(vertices.shape)
    if len(shape) not in (3, 4) or shape[-2:] != (V, 3):
        raise A2PError(f"vertices must be [B, T, {V}, 3] or [N, {V}, 3] (got {list(shape)})")
    outputs = tuple(outputs)
    unknown = [o for o in outputs if o not in OUTPUTS]
    if unknown or not outputs:
        raise A2PError(f"outputs {list(unknown or outputs)}: choose from {sorted(OUTPUTS)}")
    if surface.V != V or surface.F != rasterizer.F:
        raise A2PError(f"the surface has V={surface.V}, F={surface.F}; the rasterizer V={V}, F={rasterizer.F}")
    if int(max_bytes) < 1:
        raise A2PError(f"max_bytes={max_bytes}: need a positive byte budget")
    lead = shape[:-2]
    verts = BodyRasterizer._tensor(vertices.reshape(-1, V, 3), "vertices", f"[N, {V}, 3]", lambda s: True)
    N, dev = verts.shape[0], verts.device
    K, k_per = rasterizer._camera(K, "K", 3, N, dev)
    Rt, rt_per = rasterizer._camera(Rt, "Rt", 4, N, dev)
    want_cos, want_normals = "view_cos" in outputs, "normals" in outputs
    if want_cos:
        camera_pos = camera_centre(Rt) if camera_pos is None else camera_pos
        camera_pos = BodyRasterizer._tensor(camera_pos, "camera_pos", f"[{N} or 1, 3]", lambda s: len(s) == 2 and s[1] == 3 and s[0] in (1, N))
    channels = (3 if want_normals else 0) + (1 if want_cos else 0) + (3 if "positions" in outputs else 0)
    if s == 1:
        per_frame = 4 * (3 * V + 7 * H * W + 4 * V + channels * (V + H * W))     # proj, key + face + bary + depth, normals + cos, values + image
    else:                                                                     # proj, the s x s keys, alpha + depth, normals + cos, values + image
        per_frame = 4 * (3 * V + 2 * s * s * H * W + 2 * H * W + 4 * V + max(channels, 3) * (V + H * W))
    step = max(1, int(max_bytes) // per_frame)
    out = {o: torch.empty(N, OUTPUTS[o], H, W, dtype=torch.float32, device=dev) for o in outputs}
    for a in range(0, N, step):
        b = min(N, a + step)
        part = lambda x, per: x[a:b] if per else x
        frag = rasterizer.rasterize(verts[a:b], part(K, k_per), part(Rt, rt_per)) if s == 1 else None
        values = {"positions": verts[a:b]}
        if want_cos:
            values["normals"], cos = surface.normals_and_view_cos(verts[a:b], part(camera_pos, camera_pos.shape[0] == N and N != 1))
            values["view_cos"] = cos[:, :, None]
        elif want_normals:
            values["normals"] = surface.normals(verts[a:b])
        names = [o for o in ("normals", "view_cos", "positions") if o in outputs]
        if s > 1:                                                             # one fused launch: the positions stand in when only depth / mask are wanted
            aa = rasterizer.interpolate_antialiased(verts[a:b], torch.cat([values[o] for o in names or ["positions"]], dim=2),
                                                    part(K, k_per), part(Rt, rt_per), s, max_bytes)
            image = aa["values"]
            frag = {"depth": aa["depth"][:, 0]}
        elif names:                                                           # one interpolate launch over the concatenated channels
            image = rasterizer.interpolate(frag, torch.cat([values[o] for o in names], dim=2))
        if names:
            c = 0
            for o in names:
                out[o][a:b] = image[:, c:c + OUTPUTS[o]]
                c += OUTPUTS[o]
        if "depth" in outputs:
            out["depth"][a:b] = frag["depth"][:, None]
        if "mask" in outputs:
            out["mask"][a:b] = rasterizer.mask(frag) if s == 1 else aa["alpha"]
    return {o: x.reshape(*lead, OUTPUTS[o], H, W) for o, x in out.items()}


# ------------------------------------------------------------------------------------------------ command line
def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m audio2photoreal_amd.render",
                                 description="Depth, normal and view-cosine images of the posed vertices of a geometry.npy.")
    ap.add_argument("--geometry", required=True, help="geometry.npy of audio2photoreal_amd.skinning (key `vertices` [B, T, V, 3])")
    ap.add_argument("--assets", required=True, help="static_assets.pt: topology with vi, vt, vti, v2uv")
    ap.add_argument("--out", required=True, help="frames.npy: a pickled dict of float32 arrays [B, T, C, H, W]")
    ap.add_argument("--outputs", nargs="+", default=["depth", "normals", "view_cos", "mask"], choices=sorted(OUTPUTS),
                    help="with --supersample above 1 the mask is the coverage and the other images are premultiplied by it")
    avatar.add_camera_arguments(ap, eye_help="in front of the vertices' bounding box along +z, far enough to see all of it")
    avatar.add_render_arguments(ap, png="<output>", background=False)
    return ap


def _camera_from_args(args, verts: np.ndarray, H: int, W: int):
    if args.camera_json is not None:
        if args.target is not None:
            raise A2PError("--target goes with --eye, not with --camera-json")
        spec = json.load(open(args.camera_json))
        K, Rt = np.asarray(spec["K"], np.float32), np.asarray(spec["Rt"], np.float32)
        return torch.from_numpy(K.reshape(-1, 3, 3)), torch.from_numpy(Rt.reshape(-1, 3, 4))
    lo, hi = verts.reshape(-1, 3).min(0), verts.reshape(-1, 3).max(0)
    target = np.asarray(args.target, np.float64) if args.target is not None else (lo + hi) / 2
    if args.eye is not None:
        eye = np.asarray(args.eye, np.float64)
    else:
        half = np.radians(args.fov) / 2
        reach = max((hi[1] - lo[1]) / 2, (hi[0] - lo[0]) / 2 * H / W, 1e-6) / np.tan(half)
        eye = target + np.array([0.0, 0.0, 1.1 * reach + (hi[2] - lo[2]) / 2])
    K, Rt = look_at(eye, target, args.up, H, W, args.fov)
    return K[None], Rt[None]


def write_pngs(images: dict, directory: str, first: int = 0) -> int:
    """<name>_<sequence>_<frame>.png for every frame of every image: normals as 127.5 (1 + n) (black background), the view cosine
    as grey 255 |cos|, the mask as 0 / 255, depth as grey from white (nearest) to dark (farthest) over the clip, positions scaled
    to their bounding box; a uint8 image is written as it is.  `first`: the number of the first frame.  Returns the number of files."""
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    count = 0
    covered = {k: v != 0 for k, v in images.items()}
    for name, x in images.items():
        x = x.reshape((-1,) + x.shape[-4:]) if x.ndim == 5 else x[None]
        hit = covered[name].reshape(x.shape).any(2, keepdims=True)
        if x.dtype == np.uint8:
            pix = x
        elif name == "normals":
            pix = 127.5 * (1.0 + x) * hit
        elif name in ("view_cos", "mask"):
            pix = 255.0 * np.abs(x)
        else:
            lo = np.where(hit, x, np.inf).min(axis=(0, 1, 3, 4), keepdims=True) if hit.any() else 0.0
            hi = np.where(hit, x, -np.inf).max(axis=(0, 1, 3, 4), keepdims=True) if hit.any() else 1.0
            unit = (x - lo) / np.maximum(hi - lo, 1e-12)
            pix = 255.0 * (0.15 + 0.85 * (1.0 - unit) if name == "depth" else unit) * hit
        pix = np.clip(np.rint(pix), 0, 255).astype(np.uint8)
        for b in range(pix.shape[0]):
            for t in range(pix.shape[1]):
                frame = pix[b, t]
                img = Image.fromarray(frame[0], "L") if frame.shape[0] == 1 else Image.fromarray(np.ascontiguousarray(frame.transpose(1, 2, 0)), "RGB")
                img.save(os.path.join(directory, f"{name}_{b:02d}_{first + t:05d}.png"))
                count += 1
    return count


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    H, W = args.size
    verts = avatar.load_vertices(args.geometry, args.frames)
    avatar.require_gpu("the images are rendered")
    surface = BodySurface.from_static_assets(torch.load(args.assets, map_location="cpu", weights_only=False))
    rasterizer = BodyRasterizer(surface, H, W)
    K, Rt = _camera_from_args(args, verts, H, W)
    out = render_motion(rasterizer, surface, torch.from_numpy(np.ascontiguousarray(verts)).to("cuda"), K.to("cuda"), Rt.to("cuda"),
                        outputs=args.outputs, max_bytes=args.max_bytes, supersample=args.supersample)
    images = {k: v.cpu().numpy() for k, v in out.items()}
    np.save(args.out, images)
    print(f"{args.out}: " + ", ".join(f"{k} {list(v.shape)}" for k, v in images.items()))
    if args.png_dir is not None:
        print(f"{args.png_dir}: {write_pngs(images, args.png_dir)} png files")
    return 0


if __name__ == "__main__":
    sys.exit(main())
