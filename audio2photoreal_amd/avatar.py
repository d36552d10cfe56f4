"""The front end the avatar stages share -- skinning, surface, render, decoder, texture, encoder, scene and video -- written once:
host preparation of weights and assets, the checks that turn a clip into per-frame operands on the MI355X, the chunk loop over
frames, and the command-line kit of the stages' `parser()` and `main()`.  Nothing here launches a kernel of its own; a stage
module imports this one at its top, and this one imports a stage module only inside the function that needs it."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import A2PError


# ------------------------------------------------------------------------------------------------ host preparation
def as_numpy(a) -> np.ndarray:
    return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)


def f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32)


def asset(assets, key: str, needed=None):
    """assets[key] or assets.key; a ValueError names the missing key and, when `needed` is given, the keys the caller reads."""
    if hasattr(assets, "keys") and key in assets:
        return assets[key]
    if hasattr(assets, key):
        return getattr(assets, key)
    raise ValueError(f"the assets hold no `{key}`" + (f" (needed: {', '.join(needed)})" if needed else ""))


def checked(state_dict, key: str, shape) -> np.ndarray:
    """float32 state_dict[key], or a ValueError naming the missing key, the wrong shape or the first value that is not finite."""
    if key not in state_dict:
        raise ValueError(f"the state dict has no `{key}` (expected shape {list(shape)})")
    a = as_numpy(state_dict[key])
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f"`{key}` has shape {list(a.shape)}; the configuration expects {list(shape)}")
    bad = np.argwhere(~np.isfinite(a))
    if bad.size:
        raise ValueError(f"`{key}`{list(map(int, bad[0]))} is not finite ({a[tuple(bad[0])]})")
    return np.ascontiguousarray(a, np.float32)


def resize_axis_half64(n_in: int, n_out: int):
    """(i0, i1, weight of i1) float64 of F.interpolate's bilinear rule with align_corners=False along one axis."""
    src = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    return i0, i0 + (i0 < n_in - 1), src - i0


class HostNet:
    """Host arrays in `params` (under the reference's key names for a network's folded float32 weights); device copies are made on
    first use, per device, and kept in `_dev`.  A network is built by its from_state_dict."""

    def __init__(self):
        raise TypeError(f"use {type(self).__name__}.from_state_dict")

    def _tables(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in self.params.items()}
        return self._dev[key]


def gpu_f32(x, name: str, shape: str, ok):
    """x, a float32 tensor on the GPU whose shape `ok` accepts; A2PError says `shape` otherwise."""
    if not torch.is_tensor(x):
        raise A2PError(f"{name} must be a tensor on the MI355X (got {type(x).__name__})")
    _lib.require_gpu_tensor(x, name)
    if x.dtype != torch.float32 or not ok(tuple(x.shape)):
        raise A2PError(f"{name} must be float32 {shape} (got {x.dtype} {list(x.shape)})")
    return x


def operand(t, name: str, shape_text: str, ok, dev):
    """gpu_f32 of a launch's operand beside x: on x's device, contiguous."""
    t = gpu_f32(t, name, shape_text, ok)
    if t.device != dev:
        raise A2PError(f"{name} is on {t.device}, x on {dev}")
    return t.contiguous()


def source(x, name: str):
    """(tensor kept alive, A2PConvSource): [N, C, H, W] float32 on the GPU whose planes are dense; the frames may be further apart
    than C H W (a channel window x[:, a:b] of a contiguous tensor is passed as it is), anything else is made contiguous."""
    x = gpu_f32(x, name, "[N, C, H, W] with C, H, W >= 1", lambda s: len(s) == 4 and min(s[1:]) >= 1)
    N, C, H, W = x.shape
    dense = x.stride(3) == 1 and x.stride(2) == W and x.stride(1) == H * W and (N <= 1 or x.stride(0) >= C * H * W)
    if not dense:
        x = x.contiguous()
    return x, _lib.A2PConvSource(_lib.ptr(x), x.stride(0) if N > 1 else C * H * W, C, H, W, 0)


# ------------------------------------------------------------------------------------------------ the clip front
def clip_frames(entry_name: str, poses, P_pos: int, device=None):
    """(frames [N, P_pos] float32 on the GPU, the leading axes) of un-normalised body motion in the layouts
    skinning.motion_frames takes.  A host array goes to `device` (default: the current GPU)."""
    from .skinning import motion_frames
    frames, lead = motion_frames(poses, P_pos)
    if not torch.is_tensor(frames):
        frames = torch.from_numpy(frames)
    if not frames.is_cuda:
        if not torch.cuda.is_available():
            raise A2PError(f"{entry_name} runs on the MI355X; there is no CPU implementation")
        frames = frames.to(device if device is not None else "cuda")
    return frames, lead


def per_frame(x, name: str, lead, trailing_shape, dev):
    """x [*lead, *trailing_shape] (array or tensor) as a contiguous float32 [N, *trailing_shape] on dev."""
    x = torch.as_tensor(x)
    if tuple(x.shape) != (*lead, *trailing_shape):
        raise A2PError(f"{name} must be {[*lead, *trailing_shape]} (got {list(x.shape)})")
    return x.to(device=dev, dtype=torch.float32).reshape(math.prod(lead), *trailing_shape).contiguous()


def cameras(K, Rt, camera_pos, dev):
    """(K [C, 3, 3], Rt [C, 3, 4], camera_pos [C, 3], C) float32 on dev: C >= 1 cameras shown side by side; camera_pos defaults to
    render.camera_centre(Rt)."""
    from .render import camera_centre
    K = torch.as_tensor(K).to(device=dev, dtype=torch.float32)
    Rt = torch.as_tensor(Rt).to(device=dev, dtype=torch.float32)
    if K.dim() != 3 or K.shape[1:] != (3, 3) or Rt.dim() != 3 or Rt.shape[1:] != (3, 4) or K.shape[0] != Rt.shape[0] or K.shape[0] < 1:
        raise A2PError(f"K must be [C, 3, 3] and Rt [C, 3, 4] with C >= 1 cameras (got {list(K.shape)} and {list(Rt.shape)})")
    C = K.shape[0]
    camera_pos = camera_centre(Rt) if camera_pos is None else torch.as_tensor(camera_pos).to(device=dev, dtype=torch.float32)
    if tuple(camera_pos.shape) != (C, 3):
        raise A2PError(f"camera_pos must be [{C}, 3] (got {list(camera_pos.shape)})")
    return K, Rt, camera_pos, C


def check_pose_width(skeleton, decoder, prefix: str = ""):
    if skeleton.P_pos != 6 + decoder.n_pose_dims:
        raise A2PError(f"{prefix}the skeleton takes {skeleton.P_pos} pose parameters; the decoder 6 + n_pose_dims = {6 + decoder.n_pose_dims}")


def check_embedding_widths(body_encoder, face_encoder, decoder, prefix: str = ""):
    if (body_encoder.n_embs, face_encoder.n_embs) != (decoder.n_embs, decoder.n_face_embs):
        raise A2PError(f"{prefix}the encoders give {body_encoder.n_embs} / {face_encoder.n_embs} embedding values; the decoder takes "
                       f"{decoder.n_embs} / {decoder.n_face_embs}")


def check_body_embs(body_embs):
    if body_embs not in ("per_frame", "rest"):
        raise A2PError(f"body_embs={body_embs!r}: need 'per_frame' or 'rest'")


# ------------------------------------------------------------------------------------------------ the chunk loop
def frame_chunks(N: int, max_bytes: int, bytes_per_frame: int):
    """(a, b) of the chunks of max(1, max_bytes // bytes_per_frame) frames that tile [0, N) in order."""
    chunk = max(1, int(max_bytes) // int(bytes_per_frame))
    for a in range(0, N, chunk):
        yield a, min(N, a + chunk)


def decode_and_pose(decoder, skeleton, frames, embs, face_embs):
    """(BodyDecoder.forward's dict, posed vertices [N, V, 3]) of a chunk: the decoded displacement goes to the skeleton as
    verts_unposed."""
    preds = decoder.forward(frames, embs, face_embs)
    return preds, skeleton.pose_vertices(frames, verts_unposed=preds["geom_delta_rec"])


def uint8_panel(image):
    """Display RGB [N, 3, H, W] as uint8 [N, H, W, 3]: clipped to [0, 255] and truncated."""
    return image.permute(0, 2, 3, 1).clip(0, 255).to(torch.uint8)


# ------------------------------------------------------------------------------------------------ the command-line kit
DECODER_FLAGS = (("n-pose-enc-channels", 16), ("n-embs", 1024), ("n-embs-enc-channels", 32), ("n-face-embs", 256),
                 ("n-init-channels", 64), ("n-min-channels", 4))
EYE_HELP = "in front of the first frame's bounding box along +z, far enough to see all of it"


def add_camera_arguments(ap, per: str = "frame", eye_help: str = EYE_HELP):
    """--camera-json | --eye, --target, --up and --fov, what render._camera_from_args reads.  `per`: what a list in the JSON file
    holds one camera for.  Returns the mutually exclusive group."""
    cam = ap.add_mutually_exclusive_group()
    cam.add_argument("--camera-json", metavar="FILE", help=f'{{"K": 3 x 3, "Rt": 3 x 4}} (OpenCV), or lists of them, one per {per}')
    cam.add_argument("--eye", type=float, nargs=3, metavar=("X", "Y", "Z"), help=f"camera position; default: {eye_help}")
    ap.add_argument("--target", type=float, nargs=3, metavar=("X", "Y", "Z"), help="point looked at; default: the bounding box centre")
    ap.add_argument("--up", type=float, nargs=3, default=(0.0, 1.0, 0.0), metavar=("X", "Y", "Z"), help="world direction shown upwards")
    ap.add_argument("--fov", type=float, default=40.0, help="vertical field of view in degrees")
    return cam


def add_network_arguments(ap, decoder_only: bool = False, encoders: bool = False):
    """The configuration load_avatar reads: the body decoder's alone (decoder_only), with the texture networks', and with the
    encoders' (--encoder-uv-size and --body-embs)."""
    flags = [("uv-size", 1024)]
    if decoder_only:
        ap.add_argument("--prefix", default="decoder.")
        flags += [("init-uv-size", 64), ("n-pose-dims", 98)]
    else:
        flags += [("n-init-ftrs", 8), ("upscale-n-ftrs", 8), ("pose-to-shadow-dims", 104)]
    if encoders:
        flags.append(("encoder-uv-size", 512))
        ap.add_argument("--body-embs", choices=("per_frame", "rest"), default="per_frame",
                        help="rest: encode the template once (not the reference's loop)")
    for name, default in (*flags, *DECODER_FLAGS):
        ap.add_argument(f"--{name}", type=int, default=default)


def add_render_arguments(ap, png=None, background: bool = True):
    """--size, --frames, --max-bytes, --supersample; --png-dir when `png` names the files; --background unless switched off."""
    ap.add_argument("--size", type=int, nargs=2, default=(256, 256), metavar=("H", "W"), help="height and width of the image (of one camera's panel)")
    ap.add_argument("--frames", default=None, metavar="A:B", help="frames A..B-1 of the time axis only")
    if png is not None:
        ap.add_argument("--png-dir", default=None, metavar="DIR", help=f"also write {png}_<sequence>_<frame>.png per frame")
    ap.add_argument("--max-bytes", type=int, default=1 << 30, help="byte budget of one chunk of frames")
    ap.add_argument("--supersample", type=int, default=1, metavar="S", choices=range(1, _lib.RENDER_MAX_SUPERSAMPLE + 1),
                    help="anti-aliasing: S x S samples per pixel")
    if background:
        ap.add_argument("--background", type=float, nargs=3, default=None, metavar=("R", "G", "B"),
                        help="display colour in [0, 255] behind the avatar, in every panel (default: black, the linear image's 0)")


def add_video_arguments(ap):
    ap.add_argument("--video", default=None, metavar="FILE", help="also write a Motion-JPEG AVI file, encoded on the GPU (video.py); several "
                    "sequences go to <stem>_<r>.avi")
    ap.add_argument("--audio", default=None, metavar="FILE", help="with --video: the recording's wav file, every channel written as 16-bit PCM")
    ap.add_argument("--fps", type=float, default=30.0, help="with --video: frames per second")


def video_audio(args):
    """(samples, rate) of --audio, (None, None) without it."""
    from .video import wav_audio
    return wav_audio(args.audio) if args.audio is not None else (None, None)


def frame_window(text) -> slice:
    """The slice of --frames A:B; either end may be left out, and None is the whole axis."""
    a, _, b = (text or ":").partition(":")
    return slice(int(a) if a else None, int(b) if b else None)


def require_gpu(what: str):
    if not torch.cuda.is_available():
        raise A2PError(f"{what} on the MI355X; there is no CPU implementation")


def load_block(path: str, *keys, hint: str = ""):
    """The entries `keys` of the pickled dict in the .npy file `path`, as a list; a key given as a tuple of names stands for the
    first of them the file holds.  A2PError names what is missing and the keys there are."""
    block = np.load(path, allow_pickle=True).item()
    out = []
    for key in keys:
        names = key if isinstance(key, tuple) else (key,)
        found = [n for n in names if n in block]
        if not found:
            what = f"no `{names[0]}`" if len(names) == 1 else "neither " + " nor ".join(f"`{n}`" for n in names)
            raise A2PError(f"{path} holds {what} (keys: {sorted(block)}){hint}")
        out.append(block[found[0]])
    return out


def load_vertices(path: str, frames=None) -> np.ndarray:
    """float32 `vertices` [B, T, V, 3] or [N, V, 3] of a geometry.npy, the window --frames of its time axis."""
    (verts,) = load_block(path, "vertices", hint="; run the skinning command without --joints-only")
    verts, window = np.asarray(verts, np.float32), frame_window(frames)
    return verts[:, window] if verts.ndim == 4 else verts[window]


def load_motion_clip(results: str, embeddings: str, frames=None):
    """(motions [B, T, P], embs [B, T, .], face_embs [B, T, .]) float32 of a results.npy (`motions` [B, P, 1, T] or [B, T, P]) and
    the .npz beside it, the window --frames of their time axis."""
    (motions,) = load_block(results, ("motions", "motion"))
    motions = np.asarray(motions, np.float32)
    e = np.load(embeddings)
    for key in ("embs", "face_embs"):
        if key not in e.files:
            raise A2PError(f"{embeddings} holds no `{key}` (keys: {sorted(e.files)})")
    embs, face_embs = np.asarray(e["embs"], np.float32), np.asarray(e["face_embs"], np.float32)
    if motions.ndim == 4:
        motions = np.ascontiguousarray(motions[:, :, 0].transpose(0, 2, 1))               # [B, T, P]
    window = frame_window(frames)
    return motions[:, window], embs[:, window], face_embs[:, window]


def load_codes_clip(path: str):
    """float32 (`pose`, `face`) of a results.npy of sampler output, un-normalised."""
    pose, face = load_block(path, "pose", "face")
    return np.asarray(pose, np.float32), np.asarray(face, np.float32)


class Avatar(NamedTuple):
    """One person's networks and mesh, as encoder.render_codes_motion takes them; `surface` is the BodySurface the scene rasterises."""
    face_decoder: object
    face_encoder: object
    body_encoder: object
    decoder: object
    texture: object
    skeleton: object
    surface: object


def load_avatar(assets_path: str, checkpoint_path: str, args) -> Avatar:
    """The networks of one person from static_assets.pt and the body model's state dict, configured by the flags of
    add_network_arguments; what the command's parser has no flags for -- the texture, the encoders -- is None."""
    from .decoder import BodyDecoder
    from .encoder import BodyEncoder, FaceDecoder, FaceEncoder
    from .skinning import BodySkeleton
    from .surface import BodySurface
    from .texture import BodyTexture
    assets = torch.load(assets_path, map_location="cpu", weights_only=False)
    state = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    surface = BodySurface.from_static_assets(assets, uv_size=args.uv_size)
    decoder_only = not hasattr(args, "pose_to_shadow_dims")
    own = dict(prefix=args.prefix, init_uv_size=args.init_uv_size, n_pose_dims=args.n_pose_dims) if decoder_only else \
        dict(n_pose_dims=args.pose_to_shadow_dims - 6)
    decoder = BodyDecoder.from_state_dict(
        state, assets, surface, uv_size=args.uv_size, n_pose_enc_channels=args.n_pose_enc_channels, n_embs=args.n_embs,
        n_embs_enc_channels=args.n_embs_enc_channels, n_face_embs=args.n_face_embs, n_init_channels=args.n_init_channels,
        n_min_channels=args.n_min_channels, **own)
    texture = None if decoder_only else BodyTexture.from_state_dict(
        state, assets, surface, uv_size=args.uv_size, n_init_ftrs=args.n_init_ftrs, upscale_n_ftrs=args.upscale_n_ftrs,
        pose_to_shadow_dims=args.pose_to_shadow_dims)
    faces = (None, None, None)
    if hasattr(args, "encoder_uv_size"):
        faces = (FaceDecoder.from_state_dict(state, assets), FaceEncoder.from_state_dict(state, assets, uv_size=args.encoder_uv_size),
                 BodyEncoder.from_state_dict(state, assets, surface, uv_size=args.encoder_uv_size))
    return Avatar(*faces, decoder, texture, BodySkeleton.from_static_assets(assets), surface)
