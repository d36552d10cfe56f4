"""Surface maps of the posed body mesh on the MI355X: normals, view cosine and UV maps -- the second stage of the reference's
renderer (visualize/ca_body/utils/geom.py: vert_normals, compute_view_cos, values_to_uv, sample_uv, and the index / barycentric
images its GeometryModule gets from pytorch3d's rasteriser), as HIP launches for all frames (csrc/kernels_surface.h).

    python -m audio2photoreal_amd.surface --geometry geometry.npy --assets static_assets.pt --out surface.npy [--uv-size 256]
                                          [--camera x y z] [--frames A:B]

`BodySurface` is built once from the topology the reference reads (`from_static_assets`) or from arrays (`from_arrays`).
Construction is host work: it validates the indices, builds the vertex-to-face incidence table and the vertex-to-texture table
(the reference's compute_v2uv), and rejects anything a kernel could not index safely.  The UV index and barycentric images are
rasterised on the GPU on first use; `with_images` takes given ones instead (the reference's checkpoint holds inpainted maps).  The
methods take float32 tensors that live on the GPU and run on the caller's current stream; there is no CPU path."""
from __future__ import annotations

import argparse
import copy
import sys

import numpy as np
import torch

from . import _lib, avatar
from ._lib import A2PError


# ------------------------------------------------------------------------------------------------ host preparation
def index_array(name: str, a, cols: int, bound: int, what: str, lowest: int = 0) -> np.ndarray:
    """[., cols] int64 with every entry inside [lowest, bound), or a ValueError naming the first offending element."""
    raw = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    if raw.ndim != 2 or raw.shape[1] != cols or not (np.issubdtype(raw.dtype, np.integer) or raw.size == 0):
        raise ValueError(f"{name} must be an integer array [., {cols}] (got {raw.dtype} {list(raw.shape)})")
    out = raw.astype(np.int64)
    bad = np.argwhere((out < lowest) | (out >= bound))
    if bad.size:
        i, k = map(int, bad[0])
        raise ValueError(f"{name}[{i}, {k}] = {int(out[i, k])} is outside [{lowest}, {what}={bound})")
    return np.ascontiguousarray(out)


def incidence_table(n_verts: int, vi):
    """(inc_ptr [V + 1], inc_face) int64: the faces of vertex v are inc_face[inc_ptr[v]:inc_ptr[v + 1]], ascending in the face and
    then the corner.  A face that lists a vertex twice contributes two entries; a vertex no face uses has an empty range."""
    flat = np.asarray(vi, np.int64).reshape(-1)                                # entry 3 f + k: corner k of face f
    order = np.argsort(flat, kind="stable")                                   # stable: (face, corner) order inside a vertex
    inc_ptr = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_verts))])
    return inc_ptr.astype(np.int64), (order // 3).astype(np.int64)


def compute_v2uv(n_verts: int, vi, vti, n_max: int = 4) -> np.ndarray:
    """[V, n_max] int64 by the reference's compute_v2uv: the sorted distinct texture indices of each vertex, the unused slots
    holding the first one.  A vertex with more than n_max, or with none, is rejected by name (the reference fails on both)."""
    pairs = np.unique(np.stack([np.asarray(vi, np.int64).reshape(-1), np.asarray(vti, np.int64).reshape(-1)], 1), axis=0)
    counts = np.bincount(pairs[:, 0], minlength=n_verts)
    if counts.max() > n_max:
        v = int(np.argmax(counts > n_max))
        raise ValueError(f"vertex {v} owns {int(counts[v])} distinct texture indices; v2uv holds at most {n_max}")
    if counts.min() == 0:
        raise ValueError(f"vertex {int(np.argmin(counts))} is used by no face: it has no texture index (pass v2uv to keep it)")
    start = np.concatenate([[0], np.cumsum(counts)])[:-1]
    out = np.repeat(pairs[start, 1][:, None], n_max, axis=1)                  # pairs are sorted by vertex, then texture index
    for k in range(1, n_max):
        has = counts > k
        out[has, k] = pairs[start[has] + k, 1]
    return out


class BodySurface:
    """A triangle mesh with a UV layout, validated and laid out for the kernels.  Host arrays live on the object; device copies
    and the rasterised images are made on first use, per device."""

    def __init__(self):
        raise TypeError("use BodySurface.from_arrays or .from_static_assets")

    @classmethod
    def from_arrays(cls, vi, vt, vti, n_verts=None, v2uv=None, uv_size: int = 1024, flip_uv: bool = False) -> "BodySurface":
        """vi [F, 3] vertex indices; vt [T, 2] texture coordinates; vti [F, 3] texture indices; v2uv [V, 4] texture indices per
        vertex (built by the reference's rule when None).  V is n_verts, else v2uv's length, else the largest index + 1.
        flip_uv rasterises with v <- 1 - v (from_uv always samples at vt as given, like the reference)."""
        self = object.__new__(cls)
        vt_np = np.asarray(vt.detach().cpu().numpy() if torch.is_tensor(vt) else vt)
        if vt_np.ndim != 2 or vt_np.shape[1] != 2 or vt_np.shape[0] < 1:
            raise ValueError(f"vt must be [T >= 1, 2] (got {list(vt_np.shape)})")
        self.vt = np.ascontiguousarray(vt_np, np.float32)
        bad = np.argwhere(~np.isfinite(self.vt))
        if bad.size:
            raise ValueError(f"vt{list(map(int, bad[0]))} is not finite ({self.vt[tuple(bad[0])]})")
        T = self.vt.shape[0]
        given = None if v2uv is None else np.asarray(v2uv.detach().cpu().numpy() if torch.is_tensor(v2uv) else v2uv)
        raw_vi = np.asarray(vi.detach().cpu().numpy() if torch.is_tensor(vi) else vi)
        V = int(n_verts) if n_verts is not None else (given.shape[0] if given is not None else int(raw_vi.max(initial=-1)) + 1)
        if V < 1:
            raise ValueError(f"the mesh has V={V} vertices; need at least 1")
        self.vi = index_array("vi", raw_vi, 3, V, "V")
        self.vti = index_array("vti", vti, 3, T, "T")
        F = self.vi.shape[0]
        if F < 1 or self.vti.shape[0] != F:
            raise ValueError(f"vi holds F={F} faces and vti {self.vti.shape[0]}; need the same F >= 1")
        self.uv_size = int(uv_size)
        if not 1 <= self.uv_size <= _lib.SURFACE_MAX_UV:
            raise ValueError(f"uv_size={self.uv_size} is outside [1, {_lib.SURFACE_MAX_UV}]")
        if given is None:
            self.v2uv = compute_v2uv(V, self.vi, self.vti)
        else:
            self.v2uv = index_array("v2uv", given, 4, T, "T")
            if self.v2uv.shape[0] != V:
                raise ValueError(f"v2uv holds {self.v2uv.shape[0]} vertices; the mesh has V={V}")
        self.inc_ptr, self.inc_face = incidence_table(V, self.vi)
        self.V, self.F, self.T, self.flip_uv = V, F, T, bool(flip_uv)
        self._given = None          # (index_image, bary_image) of with_images
        self._dev, self._img = {}, {}
        return self

    @classmethod
    def from_static_assets(cls, assets, uv_size: int = 1024) -> "BodySurface":
        """The mapping the reference's AutoEncoder.__init__ reads: assets["topology"] with vi, vt, vti and v2uv."""
        topo = assets["topology"]
        return cls.from_arrays(topo["vi"], topo["vt"], topo["vti"], v2uv=topo["v2uv"], uv_size=uv_size)

    def with_images(self, index_image, bary_image) -> "BodySurface":
        """A surface that maps through the given index_image [H, H, 3] (vertex indices, -1 where a texel has none) and bary_image
        [H, H, 3] instead of rasterising its own: the `geo_fn.index_image` / `geo_fn.bary_image` buffers of the reference's
        body_dec.ckpt, which are inpainted.  Its uv_size is H; face_index_image is None."""
        idx = np.asarray(index_image.detach().cpu().numpy() if torch.is_tensor(index_image) else index_image)
        bary = np.asarray(bary_image.detach().cpu().numpy() if torch.is_tensor(bary_image) else bary_image)
        if idx.ndim != 3 or idx.shape[0] != idx.shape[1] or idx.shape[2] != 3 or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f"index_image must be an integer array [H, H, 3] (got {idx.dtype} {list(idx.shape)})")
        H = idx.shape[0]
        if not 1 <= H <= _lib.SURFACE_MAX_UV:
            raise ValueError(f"index_image has uv_size={H}, outside [1, {_lib.SURFACE_MAX_UV}]")
        if bary.shape != idx.shape:
            raise ValueError(f"bary_image is {list(bary.shape)}; index_image is {list(idx.shape)}: need the same H")
        bad = np.argwhere((idx < -1) | (idx >= self.V))
        if bad.size:
            i, j, k = map(int, bad[0])
            raise ValueError(f"index_image[{i}, {j}, {k}] = {int(idx[i, j, k])} is outside [-1, V={self.V})")
        other = copy.copy(self)
        other.uv_size = H
        other._given = (np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(bary, np.float32))
        other._img = {}
        return other

    # -------------------------------------------------------------------------------------------- device side
    def _tables(self, device):
        key = str(device)
        if key not in self._dev:
            i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(device)
            vt_raster = self.vt.copy()
            if self.flip_uv:
                vt_raster[:, 1] = np.float32(1) - vt_raster[:, 1]
            self._dev[key] = {"vi": i32(self.vi), "vti": i32(self.vti), "inc_ptr": i32(self.inc_ptr), "inc_face": i32(self.inc_face),
                              "v2uv": i32(self.v2uv), "vt": torch.from_numpy(self.vt).to(device),
                              "vt_raster": torch.from_numpy(vt_raster).to(device)}
        return self._dev[key]

    def _images(self, device):
        """(index_image int32 [H, H, 3], bary_image float32 [H, H, 3], face_index_image int32 [H, H] or None) on `device`."""
        device = torch.device(device)
        if device.type != "cuda":
            raise A2PError(f"the UV images live on the MI355X (got device {device}); the hot path has no CPU implementation")
        key = str(device)
        if key not in self._img:
            if self._given is not None:
                self._img[key] = (torch.from_numpy(self._given[0]).to(device), torch.from_numpy(self._given[1]).to(device), None)
            else:
                t, H = self._tables(device), self.uv_size
                index = torch.empty(H, H, 3, dtype=torch.int32, device=device)
                bary = torch.empty(H, H, 3, dtype=torch.float32, device=device)
                face = torch.empty(H, H, dtype=torch.int32, device=device)
                with _lib.on_device_of(index):
                    _lib.check(_lib.load().a2p_surface_uv_index(
                        _lib.ptr(t["vt_raster"]), self.T, _lib.ptr(t["vti"]), _lib.ptr(t["vi"]), self.F, H, _lib.ptr(index),
                        _lib.ptr(bary), _lib.ptr(face), _lib.current_stream(device)), "a2p_surface_uv_index")
                self._img[key] = (index, bary, face)
        return self._img[key]

    def _current(self):
        if not torch.cuda.is_available():
            raise A2PError("the UV images are rasterised on the MI355X; there is no CPU implementation")
        return torch.device("cuda", torch.cuda.current_device())

    @property
    def index_image(self):
        """int32 [H, H, 3] on the current GPU: the three vertices of the face that covers each texel, -1 where none does."""
        return self._images(self._current())[0]

    @property
    def bary_image(self):
        """float32 [H, H, 3] on the current GPU: the barycentrics of each texel centre in its face, 0 where there is none."""
        return self._images(self._current())[1]

    @property
    def face_index_image(self):
        """int32 [H, H] on the current GPU: the face that covers each texel (-1: none); None after with_images."""
        return self._images(self._current())[2]

    @staticmethod
    def _tensor(x, name: str, shape: str, ok):
        if not torch.is_tensor(x):
            raise A2PError(f"{name} must be a tensor on the MI355X (got {type(x).__name__})")
        _lib.require_gpu_tensor(x, name)
        if x.dtype != torch.float32 or not ok(tuple(x.shape)):
            raise A2PError(f"{name} must be float32 {shape} (got {x.dtype} {list(x.shape)})")
        return x.contiguous()

    def _normals(self, verts, camera_pos, want_normals: bool, want_cos: bool):
        verts = self._tensor(verts, "verts", f"[N, {self.V}, 3]", lambda s: len(s) == 3 and s[1:] == (self.V, 3))
        N, dev = verts.shape[0], verts.device
        per_frame = 0
        if want_cos:
            camera_pos = self._tensor(camera_pos, "camera_pos", f"[{N} or 1, 3]", lambda s: len(s) == 2 and s[1] == 3 and s[0] in (1, N))
            if camera_pos.device != dev:
                raise A2PError(f"camera_pos is on {camera_pos.device}, verts on {dev}")
            per_frame = int(camera_pos.shape[0] == N and N != 1)
        t = self._tables(dev)
        normals = torch.empty(N, self.V, 3, dtype=torch.float32, device=dev) if want_normals else None
        cos = torch.empty(N, self.V, dtype=torch.float32, device=dev) if want_cos else None
        if N == 0:
            return normals, cos
        with _lib.on_device_of(verts):
            _lib.check(_lib.load().a2p_surface_normals(
                _lib.ptr(verts), N, self.V, _lib.ptr(t["vi"]), self.F, _lib.ptr(t["inc_ptr"]), _lib.ptr(t["inc_face"]),
                _lib.ptr(camera_pos) if want_cos else None, per_frame, _lib.ptr(normals), _lib.ptr(cos), _lib.current_stream(dev)),
                "a2p_surface_normals")
        return normals, cos

    def normals(self, verts):
        """[N, V, 3] = vert_normals(verts, vi): unit vertex normals (0 for a vertex without a face with area)."""
        return self._normals(verts, None, True, False)[0]

    def view_cos(self, verts, camera_pos):
        """[N, V] = compute_view_cos(verts, vi, camera_pos): the cosine between a vertex's normal and the direction from the
        camera to it.  camera_pos [N, 3] or [1, 3]."""
        return self._normals(verts, camera_pos, False, True)[1]

    def normals_and_view_cos(self, verts, camera_pos):
        """(normals [N, V, 3], view_cos [N, V]) from one launch."""
        return self._normals(verts, camera_pos, True, True)

    def to_uv(self, values):
        """[N, C, H, H] = values_to_uv(values [N, V, C], index_image, bary_image), 1 <= C <= 16.  The output takes N C H H 4
        bytes; every texel is written."""
        C_max = _lib.SURFACE_MAX_CHANNELS
        values = self._tensor(values, "values", f"[N, {self.V}, C] with 1 <= C <= {C_max}",
                              lambda s: len(s) == 3 and s[1] == self.V and 1 <= s[2] <= C_max)
        N, C, dev, H = values.shape[0], values.shape[2], values.device, self.uv_size
        index, bary, _ = self._images(dev)
        out = torch.empty(N, C, H, H, dtype=torch.float32, device=dev)
        if N == 0:
            return out
        with _lib.on_device_of(values):
            _lib.check(_lib.load().a2p_surface_to_uv(_lib.ptr(values), N, self.V, C, _lib.ptr(index), _lib.ptr(bary), H, _lib.ptr(out),
                                                     _lib.current_stream(dev)), "a2p_surface_to_uv")
        return out

    def from_uv(self, values_uv):
        """[N, V, C] = sample_uv(values_uv [N, C, H', W'], vt, v2uv): the mean over a vertex's 4 texture slots of the bilinear
        sample (align_corners, zero padding).  H' and W' are the input's own, not uv_size."""
        values_uv = self._tensor(values_uv, "values_uv", "[N, C, H', W'] with C, H', W' >= 1", lambda s: len(s) == 4 and min(s[1:]) >= 1)
        N, C, Hs, Ws = values_uv.shape
        dev = values_uv.device
        t = self._tables(dev)
        out = torch.empty(N, self.V, C, dtype=torch.float32, device=dev)
        if N == 0:
            return out
        with _lib.on_device_of(values_uv):
            _lib.check(_lib.load().a2p_surface_from_uv(_lib.ptr(values_uv), N, C, Hs, Ws, _lib.ptr(t["vt"]), self.T, _lib.ptr(t["v2uv"]),
                                                       self.V, _lib.ptr(out), _lib.current_stream(dev)), "a2p_surface_from_uv")
        return out


# ------------------------------------------------------------------------------------------------ convenience
def surface_maps(surface: BodySurface, vertices, camera_pos=None) -> dict:
    """{"normals": [.., V, 3], "position_uv": [.., 3, H, H], "normal_uv": [.., 3, H, H]} of posed vertices in the layouts
    skinning.pose_motion returns, [B, T, V, 3] or [N, V, 3] (float32 on the GPU); with camera_pos ([N, 3] or [1, 3], N = B T) also
    "view_cos" [.., V] and "view_cos_uv" [.., 1, H, H].  The UV maps come from one to_uv launch over the concatenated channels.

    The UV output takes N C H H 4 bytes with C = 6 (7 with a camera): 12.6 MB per frame at H = 1024 for every 3 channels.
    Chunking the frames is the caller's job."""
    if not torch.is_tensor(vertices):
        raise A2PError(f"vertices must be a tensor on the MI355X (got {type(vertices).__name__})")
    shape = tuple(vertices.shape)
    if len(shape) not in (3, 4) or shape[-2:] != (surface.V, 3):
        raise A2PError(f"vertices must be [B, T, {surface.V}, 3] or [N, {surface.V}, 3] (got {list(shape)})")
    lead = shape[:-2]
    verts = vertices.reshape(-1, surface.V, 3)
    if camera_pos is None:
        normals, cos = surface.normals(verts), None
        uv = surface.to_uv(torch.cat([verts, normals], dim=2))
    else:
        normals, cos = surface.normals_and_view_cos(verts, camera_pos)
        uv = surface.to_uv(torch.cat([verts, normals, cos[:, :, None]], dim=2))
    H = surface.uv_size
    out = {"normals": normals.reshape(*lead, surface.V, 3), "position_uv": uv[:, 0:3].reshape(*lead, 3, H, H),
           "normal_uv": uv[:, 3:6].reshape(*lead, 3, H, H)}
    if cos is not None:
        out["view_cos"] = cos.reshape(*lead, surface.V)
        out["view_cos_uv"] = uv[:, 6:7].reshape(*lead, 1, H, H)
    return out


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m audio2photoreal_amd.surface",
                                 description="Normals and UV maps for the posed vertices of a geometry.npy.")
    ap.add_argument("--geometry", required=True, help="geometry.npy of audio2photoreal_amd.skinning (key `vertices` [B, T, V, 3])")
    ap.add_argument("--assets", required=True, help="static_assets.pt: topology with vi, vt, vti, v2uv")
    ap.add_argument("--out", required=True, help="surface.npy: a pickled dict of float32 arrays")
    ap.add_argument("--uv-size", type=int, default=256, help="side of the UV maps (N C H H 4 bytes of output)")
    ap.add_argument("--camera", type=float, nargs=3, metavar=("X", "Y", "Z"), help="camera position: adds view_cos and view_cos_uv")
    ap.add_argument("--frames", default=None, metavar="A:B", help="frames A..B-1 of the time axis only")
    return ap


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    verts = avatar.load_vertices(args.geometry, args.frames)
    avatar.require_gpu("the surface maps run")
    surface = BodySurface.from_static_assets(torch.load(args.assets, map_location="cpu", weights_only=False), uv_size=args.uv_size)
    camera = None if args.camera is None else torch.tensor([args.camera], dtype=torch.float32, device="cuda")
    out = surface_maps(surface, torch.from_numpy(np.ascontiguousarray(verts)).to("cuda"), camera)
    np.save(args.out, {k: v.cpu().numpy() for k, v in out.items()})
    print(f"{args.out}: " + ", ".join(f"{k} {list(v.shape)}" for k, v in out.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
