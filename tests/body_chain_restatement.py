"""The body renderer end to end, as a composition of the stage restatements in the order of the reference's AutoEncoder.forward
(visualize/ca_body/models/mesh_vae_drivable.py:306-361): ConvDecoder, LBSModule.pose, UNetViewDecoder (view cosine from the camera
centre, to_uv, concatenation, UNetWB), PoseToShadow, forward_tex, RenderLayer and linear2displayBatch.  Test infrastructure: the
yardstick of tests/test_body_chain_hip.py and tests/test_body_chain_cpu.py (which gate texture.BodyTexture.forward and
texture.render_rgb_motion against it), and what tests/golden/make_golden_body_chain.py measures the reference's own wiring against.

`chain` states no formula of its own: every operation is a function of decoder_restatement, skinning_restatement,
surface_restatement, texture_restatement or render_restatement, called with `dtype`.  The float32 run against the float64 run is
the rounding error float32 arithmetic makes on the whole chain: the allowance of the stages the reference cannot provide.

`MUTANTS` names one-line miswirings of the chain; `chain(..., mutant=name, base=c)` reruns only what lies downstream of the
miswired stage and takes the rest from `base`.  A gate that lets one of them pass is not a gate."""
import numpy as np

import decoder_restatement as DR
import render_restatement as RR
import skinning_restatement as SK
import surface_restatement as SU
import texture_restatement as TR
from surface_restatement import nerr  # noqa: F401  (part of this module's surface)

SEED = 5
UV, N_FRAMES, HEIGHT, WIDTH = 256, 3, 96, 128
TEX_CFG = dict(uv_size=UV, n_init_ftrs=2, upscale_n_ftrs=3, pose_to_shadow_dims=16)
DELTA_SCALE = 0.02                          # on verts_conv.weight_g and verts_conv.bias: the sheet stays mostly a sheet
FLOOR = 2.0 ** -24
MAX_DRAWS = 20

# stage: (the stages it reads, the entries it writes)
STAGES = {"decoder": ((), ("geom_delta_rec", "tex_mean_rec")),
          "verts": (("decoder",), ("verts",)),
          "cond_view": (("decoder", "verts"), ("cond_view",)),
          "tex_view_rec": (("cond_view",), ("tex_view_rec",)),
          "shadow_map": ((), ("shadow_map",)),
          "tex_rec": (("decoder", "tex_view_rec", "shadow_map"), ("tex_rec",)),
          "raster": (("verts",), ("face", "bary", "depth", "second")),
          "render": (("tex_rec", "raster"), ("render",)),
          "rgb": (("render",), ("rgb",))}

# name: (the stages it miswires, what it does)
MUTANTS = {
    "camera_from_translation": (("cond_view",), "camera_pos = Rt[:, :, 3] instead of -R^T t"),
    "view_direction_reversed": (("cond_view",), "the view direction as camera minus vertex"),
    "view_cos_unposed": (("cond_view",), "view cosine from the unposed vertices"),
    "cond_view_swapped": (("cond_view",), "cond_view as [tex_mean_rec, view_cos_uv]"),
    "tex_mean_unblurred": (("tex_rec",), "tex_mean resized without the blur"),
    "tex_std_default": (("tex_rec",), "tex_std = 64.0 instead of the assets' tex_var"),
    "shadow_not_applied": (("tex_rec",), "the shadow map not applied"),
    "shadow_without_seam_steps": (("tex_rec",), "the shadow map applied without its seam steps"),
    "template_not_added": (("verts",), "the template not added before skinning"),
    "global_scaling_dropped": (("verts",), "global_scaling dropped"),
    "texture_v_flipped": (("render",), "the texture sampled at v <- 1 - v"),
    "cameras_rotated": (("cond_view", "raster"), "the three cameras rotated by one frame"),
}

# the outputs a test gates: name -> True when it is an image over pixels (compared over the kept pixels only)
GATED = {"verts": False, "cond_view": False, "tex_view_rec": False, "shadow_map": False, "tex_rec": False, "depth": True,
         "render": True, "rgb": True}


def _sub(state, prefix):
    return {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}


def _uv(scene, dtype):
    key = np.dtype(dtype).name
    if key not in scene["_uv"]:
        scene["_uv"][key] = SU.uv_images(scene["surf"], UV, dtype=dtype)[:2]
    return scene["_uv"][key]


def chain(scene, dtype=np.float64, mutant=None, base=None):
    """Every intermediate of one run of the renderer on `scene` (make_scene), by name: geom_delta_rec, tex_mean_rec, verts,
    cond_view, tex_view_rec, shadow_map, tex_rec, face, bary, depth, second, render, rgb.  With `mutant` the named miswiring is in
    place; with `base` (a run of the same dtype without mutant) the stages it does not reach are taken from there."""
    assert mutant is None or mutant in MUTANTS, mutant
    m = mutant
    dirty = set()
    for stage, (reads, _) in STAGES.items():                                  # in forward order: a stage after what it reads
        if base is None or (m is not None and stage in MUTANTS[m][0]) or dirty & set(reads):
            dirty.add(stage)
    c = {}
    surf, vi, skel = scene["surf"], scene["surf"]["vi"], scene["skel"]
    motion, K, Rt = scene["motion"], scene["K"], scene["Rt"]
    H, W = scene["size"]
    if m == "cameras_rotated":
        K, Rt = np.roll(K, 1, axis=0), np.roll(Rt, 1, axis=0)
    tex, assets = scene["tex_state"], scene["tex_assets"]

    def run(stage, fn):
        if stage in dirty:
            c.update(fn())
        else:
            c.update({k: base[k] for k in STAGES[stage][1]})

    def decoder():
        out = DR.decoder_forward(scene["params"], scene["cfg"], scene["assets"], surf, motion, scene["embs"], scene["face_embs"], dtype=dtype)
        return {k: out[k] for k in ("geom_delta_rec", "tex_mean_rec")}

    def verts():
        template = np.zeros_like(scene["template"]) if m == "template_not_added" else scene["template"]
        scaling = 1.0 if m == "global_scaling_dropped" else scene["global_scaling"]
        return {"verts": SK.pose_vertices(skel, motion, scene["lbs_scale"][None], c["geom_delta_rec"], template, scaling, dtype)}

    def cond_view():
        camera_pos = np.asarray(Rt, dtype)[:, :, 3] if m == "camera_from_translation" else RR.camera_centre(Rt, dtype)
        seen = np.asarray(c["geom_delta_rec"], dtype) + np.asarray(scene["template"], dtype) if m == "view_cos_unposed" else c["verts"]
        cos = SU.view_cos(seen, vi, camera_pos, dtype)
        if m == "view_direction_reversed":
            cos = -cos
        index, bary = _uv(scene, dtype)
        cos_uv = SU.to_uv(cos[..., None], index, bary, dtype)
        parts = [c["tex_mean_rec"], cos_uv] if m == "cond_view_swapped" else [cos_uv, c["tex_mean_rec"]]
        return {"cond_view": np.concatenate(parts, 1)}

    def tex_view_rec():
        return {"tex_view_rec": TR.unet_forward(_sub(tex, "decoder_view.unet."), c["cond_view"], dtype=dtype)}

    def shadow_map():
        return {"shadow_map": TR.pose_shadow_forward(_sub(tex, "pose_to_shadow."), motion, 2 * UV, dtype=dtype)}

    def tex_rec():
        mean = np.asarray(assets["tex_mean"], dtype)[None]
        mean = TR.resize(mean if m == "tex_mean_unblurred" else TR.blur(mean, 11, dtype), (2 * UV, 2 * UV), dtype)
        std = 64.0 if m == "tex_std_default" else float(assets["tex_var"])
        shadow = None if m == "shadow_not_applied" else c["shadow_map"]
        seam, seam_2k = assets["seam_data_1024"], assets["seam_data_2048"]
        if m == "shadow_without_seam_steps":                                  # forward_tex with the shadow's impaint and resamples left out
            a, b = np.asarray(c["tex_mean_rec"], dtype), np.asarray(c["tex_view_rec"], dtype)
            t = TR.seam_steps(a + b, seam, 1, dtype)
            u = TR.upscale_forward(_sub(tex, "upscale_net."), np.concatenate([a, b], 1), dtype)
            return {"tex_rec": TR.seam_steps(TR.compose(t, u, mean, std, shadow, dtype), seam_2k, 2, dtype)}
        return {"tex_rec": TR.forward_tex(_sub(tex, "upscale_net."), seam, seam_2k, mean, std, c["tex_mean_rec"], c["tex_view_rec"], shadow, dtype)}

    def raster():
        return RR.rasterize(c["verts"], vi, K, Rt, H, W, dtype=dtype, runner_up=True)

    def render():
        return {"render": RR.sample_texture(c["tex_rec"], surf["vt"], surf["vti"], c["face"], c["bary"], flip_uv=m == "texture_v_flipped", dtype=dtype)}

    def rgb():
        return {"rgb": TR.display(c["render"], dtype)}

    for stage, fn in (("decoder", decoder), ("verts", verts), ("cond_view", cond_view), ("tex_view_rec", tex_view_rec), ("shadow_map", shadow_map),
                      ("tex_rec", tex_rec), ("raster", raster), ("render", render), ("rgb", rgb)):
        run(stage, fn)
    c.update(vi=vi, K=np.asarray(scene["K"]), Rt=np.asarray(scene["Rt"]), size=(H, W))     # what `excluded` needs of the scene
    return c


# ------------------------------------------------------------------------------------------------ the scene, as data
CAMERAS = (((0.3, 0.2), 1.3, (0.0, 0.0), 40.0),          # (eye offset x, y; eye distance and target offset in extents; fov)
           ((-0.45, 0.25), 1.15, (0.05, -0.04), 46.0),   # frame 0's x, y are absolute, the others in extents: off the sheet's normal
           ((0.55, -0.3), 1.4, (-0.04, 0.05), 34.0))


def draw_scene(seed=SEED, draw=0):
    """Draw `draw` of the scene: the decoder fixture (uv 256, 437 vertices) with verts_conv scaled by DELTA_SCALE, a small
    BodyTexture state at uv 256 -> 512, the 6-joint skeleton with the fixture mesh as template and global_scaling 10, 3 frames of
    gentle motion and one 96 x 128 camera per frame with its own eye, target and field of view.  Every number comes from legacy
    RandomState streams, which numpy freezes: the result is data."""
    f = DR.make_fixture()
    params = dict(f["params"])
    for k in ("verts_conv.weight_g", "verts_conv.bias"):
        params[k] = (params[k] * np.float32(DELTA_SCALE)).astype(np.float32)
    tex_state, tex_assets = TR.texture_state(41, UV, n_init_ftrs=TEX_CFG["n_init_ftrs"], upscale_n_ftrs=TEX_CFG["upscale_n_ftrs"],
                                             pose_dims=TEX_CFG["pose_to_shadow_dims"])
    tex_assets["seam_data_1024"] = f["assets"]["seam_data_1024"]              # one table at uv_size for decoder and texture, as in the reference
    skel = SK.make_skeleton(12, 6, 437, 4, P_pos=16, P_scale=3)
    rs = np.random.RandomState([seed, draw])
    motion = rs.randn(N_FRAMES, 16)
    amplitude = rs.uniform(0.85, 1.15)                                        # gentle: the random skeleton folds the sheet otherwise
    motion[:, :3] *= 0.2
    motion[:, 3:6] *= 0.18 * amplitude
    motion[:, 6:] *= 0.12 * amplitude
    scene = {"cfg": f["cfg"], "params": params, "assets": f["assets"], "surf": f["surf"], "tex_state": tex_state, "tex_assets": tex_assets,
             "tex_cfg": dict(TEX_CFG), "skel": skel, "template": f["surf"]["rest"], "lbs_scale": np.zeros(3, np.float32),
             "global_scaling": np.float32(10.0), "motion": motion.astype(np.float32), "embs": rs.randn(N_FRAMES, 16).astype(np.float32),
             "face_embs": rs.randn(N_FRAMES, 8).astype(np.float32), "size": (HEIGHT, WIDTH), "draw": int(draw), "seed": int(seed), "_uv": {}}
    posed = SK.pose_vertices(skel, scene["motion"], scene["lbs_scale"][None], None, scene["template"], scene["global_scaling"])
    Ks, Rts = [], []
    for n, ((ox, oy), distance, (tx, ty), fov) in enumerate(CAMERAS):
        lo, hi = posed[n].min(0), posed[n].max(0)
        centre, extent = (lo + hi) / 2, float((hi - lo).max())
        unit = 1.0 if n == 0 else extent
        eye = centre + np.array([ox * unit, oy * unit, distance * extent]) + rs.uniform(-0.03, 0.03, 3) * extent
        target = centre + np.array([tx, ty, 0.0]) * extent + rs.uniform(-0.01, 0.01, 3) * extent
        K, Rt = RR.look_at(eye, target, (0.0, 1.0, 0.0), HEIGHT, WIDTH, fov + rs.uniform(-1, 1), np.float32)
        Ks.append(K)
        Rts.append(Rt)
    scene["K"], scene["Rt"] = np.asarray(Ks, np.float32), np.asarray(Rts, np.float32)
    return scene


def make_scene(seed=SEED, accept=None, log=print):
    """The first draw of draw_scene(seed, .) that `accept` takes; by default the one whose float64 and float32 chains meet the
    conditions of `conditions` (about half a minute a draw).  Mutants are judged by the golden maker, which has the reference's
    errors.  Returns (scene, what accept returned)."""
    def default(scene):
        c64, c32 = chain(scene), chain(scene, np.float32)
        y = yardsticks(c64, c32)
        ex = excluded(c64, y["e_proj"], y["e_depth"])
        facts = conditions(c64, ex)
        same = np.array_equal(c32["face"][~ex], c64["face"][~ex])
        log(f"draw {scene['draw']}: {facts}, float32 faces equal outside excluded: {same}")
        return {"c64": c64, "c32": c32, "yardsticks": y, "excluded": ex, "conditions": facts} if same and not failed(facts) else None

    accept = default if accept is None else accept
    for draw in range(MAX_DRAWS):
        scene = draw_scene(seed, draw)
        got = accept(scene)
        if got:
            return scene, got
    raise SystemExit(f"no draw out of {MAX_DRAWS} met the conditions")


def fingerprints(scene):
    """{name: float64 sum}: every array of the scene's state dicts, skeleton, inputs and cameras."""
    out = {}
    for group in ("params", "tex_state", "skel"):
        out.update({f"{group}/{k}": float(np.asarray(v, np.float64).sum()) for k, v in scene[group].items()})
    for k in ("motion", "embs", "face_embs", "K", "Rt", "template"):
        out[f"input/{k}"] = float(np.asarray(scene[k], np.float64).sum())
    out["input/tex_mean"] = float(np.asarray(scene["tex_assets"]["tex_mean"], np.float64).sum())
    return out


# ------------------------------------------------------------------------------------------------ yardsticks, exclusions, conditions
def over(x, mask):
    """The values of an image [N, H, W] or [N, C, H, W] at the pixels of mask [N, H, W]."""
    x = np.asarray(x)
    return x[mask] if x.ndim == 3 else x.transpose(0, 2, 3, 1)[mask]


def excluded(chain64, e_proj, e_depth):
    """bool [N, H, W], from the float64 chain alone: the pixels on whose face float32 and float64 may disagree.  A pixel is excluded
    when its centre lies within CLEARANCE_FACTOR x e_proj (pixels) of a projected edge of a kept face of its frame, or when it is
    covered and its runner-up's depth is within CLEARANCE_FACTOR x e_depth (relative) of the winner's."""
    c = chain64
    H, W = c["size"]
    near_edge = RR.edge_distance(c["verts"], c["vi"], c["K"], c["Rt"], H, W) <= RR.CLEARANCE_FACTOR * float(e_proj)
    hit = c["face"] >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = (c["second"] - c["depth"]) / c["depth"]
    return near_edge | (hit & (gap <= RR.CLEARANCE_FACTOR * float(e_depth)))


def yardsticks(c64, c32):
    """The float32 chain's error against the float64 chain: e/<stage> (nerr) for every continuous stage, e_proj (pixels, the
    largest difference of a projected vertex), e_depth (relative, over the pixels whose face agrees), and e/depth, e/render and
    e/rgb over the kept pixels (covered and outside `excluded`)."""
    y = {f"e/{k}": nerr(c32[k], c64[k]) for k in ("geom_delta_rec", "tex_mean_rec", "verts", "cond_view", "tex_view_rec", "shadow_map", "tex_rec")}
    y["e/view_cos_uv"] = nerr(c32["cond_view"][:, :1], c64["cond_view"][:, :1])
    p64 = RR.project(c64["verts"], c64["K"], c64["Rt"])
    p32 = RR.project(c32["verts"], c32["K"], c32["Rt"], np.float32)
    y["e_proj"] = float(np.abs(p32[..., :2].astype(np.float64) - p64[..., :2]).max())
    same = (c64["face"] >= 0) & (c32["face"] == c64["face"])
    y["e_depth"] = float((np.abs(c32["depth"][same].astype(np.float64) - c64["depth"][same]) / c64["depth"][same]).max())
    kept = (c64["face"] >= 0) & ~excluded(c64, y["e_proj"], y["e_depth"])
    for k in ("depth", "render", "rgb"):
        y[f"e/{k}"] = nerr(over(c32[k], kept), over(c64[k], kept))
    return y


def conditions(c64, ex):
    """What part 3 of the scene's contract asks, per frame, recomputed from the float64 chain and its excluded mask: the covered
    share of the image, the excluded share of the covered pixels, the share covered twice, and the share of covered display values
    at a clamp."""
    hit = c64["face"] >= 0
    twice = hit & np.isfinite(c64["second"])
    rgb = over(c64["rgb"], hit)
    per = lambda a, b: [float(a[n].sum() / max(b[n].sum(), 1)) for n in range(len(hit))]
    return {"covered": [float(hit[n].mean()) for n in range(len(hit))], "excluded": per(ex & hit, hit), "twice": per(twice, hit),
            "clamped": float(((rgb <= 0) | (rgb >= 255)).mean())}


def failed(facts):
    """The conditions `facts` (of `conditions`) misses, as text; empty when all hold."""
    out = []
    if min(facts["covered"]) < 0.25:
        out.append(f"a frame covers {min(facts['covered']):.3f} of its image, below 0.25")
    if max(facts["excluded"]) > 0.02:
        out.append(f"excluded holds {max(facts['excluded']):.4f} of a frame's covered pixels, above 0.02")
    if min(facts["twice"]) < 0.05:
        out.append(f"only {min(facts['twice']):.3f} of a frame's covered pixels are covered twice, below 0.05")
    if facts["clamped"] > 0.5:
        out.append(f"{facts['clamped']:.3f} of the covered display values sit at a clamp, above 0.5")
    return out


def allowances(e):
    """{output: 4 max(e, 2^-24)} for the gated outputs from a mapping that holds e_ref/<stage> where the reference provides the
    stage (geom, cond_view and its view-cosine channel alone, tex_mean_rec, tex_view_rec, shadow_map) and e/<stage> for the rest."""
    pick = {"geom_delta_rec": "e/geom_delta_rec", "tex_mean_rec": "e_ref/tex_mean_rec", "view_cos_uv": "e_ref/view_cos_uv",
            "verts": "e_ref/geom", "cond_view": "e_ref/cond_view", "tex_view_rec": "e_ref/tex_view_rec", "shadow_map": "e_ref/shadow_map",
            "tex_rec": "e/tex_rec", "depth": "e/depth", "render": "e/render", "rgb": "e/rgb"}
    return {k: 4 * max(float(e[v]), FLOOR) for k, v in pick.items()}


def mutant_ratio(c64, m64, kept, allowance):
    """The largest, over the gated outputs, of the mutant's normalised distance from the chain divided by that output's allowance;
    images over the kept pixels only.  (ratio, the output that gave it)."""
    best = (0.0, "")
    for k, image in GATED.items():
        err = nerr(over(m64[k], kept), over(c64[k], kept)) if image else nerr(m64[k], c64[k])
        best = max(best, (err / allowance[k], k))
    return best
