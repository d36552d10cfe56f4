"""DPM-Solver++(2M) on the MI355X (GaussianDiffusion.dpm_solver_sample_loop, csrc/kernels_multistep.h): the stand-alone update and
one fused step against float32 restatements bit for bit, the solver's order on a problem with a closed-form denoiser, the fused loop
against the generic path and a float64 oracle loop, fp16 against fp32, held elements, windows, and the fp32 escalation repeat.
Measured numbers go to record(...)."""
import numpy as np
import pytest
import torch

from audio2photoreal_amd import _lib
from audio2photoreal_amd.model_util import create_gaussian_diffusion, create_model_and_diffusion, default_args, load_model
from audio2photoreal_amd.sample import inpaint
from audio2photoreal_amd.sample.inpaint import expand_mask, inpaint_sample_loop
from audio2photoreal_amd.sample.long_form import generate_from_long_recording, plan_windows, window_gather, windowed_sample_loop
from audio2photoreal_amd.sample.recording import continue_recording, generate_from_recording
from conftest import record, rel_l2
from test_inpaint_hip import _fma32, _masks, _models, _norm, _randn, _recording, _stats, _y
from test_multistep_cpu import _restated

pytestmark = pytest.mark.gpu
SEED = 10
SR = 44100
T = 240
PRECISIONS = ["fp32", "fp16"]
MS = "dpm++2m"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _diffusion(respacing):
    return create_gaussian_diffusion(default_args("face", timestep_respacing=respacing))


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _restated_update(x, x0, x0_prev, cf, t):
    """float32 numpy in kernels_multistep.h multistep_update's order: fmaf(CX, x, fmaf(B2, x0, P2 * x0_prev)) with history,
    fmaf(CX, x, B1 * x0) without, x0 itself at t == 0."""
    f = np.float32
    if t == 0:
        return x0.copy()
    cx, b1, b2, p2 = (f(v) for v in cf[:, t])
    full = lambda v: np.broadcast_to(np.asarray(v, f), x.shape)
    if x0_prev is None:
        return _fma32(full(cx), x, (b1 * x0).astype(f))
    return _fma32(full(cx), x, _fma32(full(b2), x0, (p2 * x0_prev).astype(f)))


# ---------------------------------------------------------------------------------------------- 1. stand-alone update

@pytest.mark.parametrize("order", [1, 2])
def test_standalone_update_matches_the_restatement(dev, order):
    d = _diffusion("ddim20")
    cf = d._multistep_coefs(dev)
    cf_h = cf.cpu().numpy()
    ts = [0, 1, 2, 7, 19]
    B, per = len(ts), 3 * 1000
    x = _randn(B, 3, 1, 1000).to(dev)
    x0 = _randn(B, 3, 1, 1000, seed=SEED + 1, scale=0.7).to(dev)
    x0[0, 0, 0, :4] = torch.tensor([-0.0, 0.0, -1e-40, 1e-40])         # signed zeros and subnormals survive the last step
    prev = _randn(B, 3, 1, 1000, seed=SEED + 2, scale=0.7).to(dev) if order == 2 else None
    t = torch.tensor(ts, dtype=torch.int64, device=dev)
    got = d._elementwise("a2p_multistep_update", x, _lib.ptr(x), _lib.ptr(x0), _lib.ptr(prev), _lib.ptr(t), _lib.ptr(cf), d.num_timesteps)
    xh, x0h = x.cpu().numpy().reshape(B, per), x0.cpu().numpy().reshape(B, per)
    ph = None if prev is None else prev.cpu().numpy().reshape(B, per)
    want = np.stack([_restated_update(xh[b], x0h[b], None if ph is None else ph[b], cf_h, ts[b]) for b in range(B)])
    assert np.array_equal(got.cpu().numpy().reshape(B, per).view(np.int32), want.view(np.int32))
    assert _bits_equal(got[0], x0[0])                                   # row 0: the sample is pred_xstart's bits
    # the documented alias: sample = x
    xa = x.clone()
    d._call("a2p_multistep_update", xa, _lib.ptr(xa), _lib.ptr(x0), _lib.ptr(prev), _lib.ptr(t), _lib.ptr(cf), d.num_timesteps, B, per,
            _lib.ptr(xa))
    assert _bits_equal(xa, got)


def test_update_refuses_an_aliased_history(dev):
    d = _diffusion("ddim20")
    cf = d._multistep_coefs(dev)
    x, x0 = torch.zeros(2, 8, device=dev), torch.zeros(2, 8, device=dev)
    t = torch.zeros(2, dtype=torch.int64, device=dev)
    with pytest.raises(_lib.A2PError, match="alias"):
        d._call("a2p_multistep_update", x, _lib.ptr(x), _lib.ptr(x0), _lib.ptr(x0), _lib.ptr(t), _lib.ptr(cf), d.num_timesteps, 2, 8,
                _lib.ptr(x))


# ---------------------------------------------------------------------------------------------- 2. order on the analytic problem

def _analytic(dev):
    """Per element x0 ~ N(mu, s^2), mu ~ 0.5 N(0, 1), s ~ U[0.2, 1.2]; 20 000 elements drawn with default_rng(0) in the order mu, s,
    x_T, laid out [2, 100, 1, 100].  E[x0 | x_t] = mu + s^2 a (x_t - a mu) / (a^2 s^2 + sigma^2), a^2 = abar of the ORIGINAL
    timestep, is returned in [B, T, C] by a plain callable (the generic path)."""
    rng = np.random.default_rng(0)
    n = 20000
    mu = 0.5 * rng.standard_normal(n)
    s = rng.uniform(0.2, 1.2, n)
    xT = rng.standard_normal(n)
    shape = (2, 100, 1, 100)
    acp = torch.from_numpy(_diffusion("").alphas_cumprod).to(dev)
    mu_d, s_d = (torch.from_numpy(v.reshape(shape)).to(dev) for v in (mu, s))

    def denoiser(x, ts, **kw):
        a2 = acp[ts].view(-1, 1, 1, 1)
        a = a2.sqrt()
        x0 = mu_d + s_d ** 2 * a * (x.double() - a * mu_d) / (a2 * s_d ** 2 + (1.0 - a2))
        return x0.float().squeeze(2).permute(0, 2, 1).contiguous()
    return denoiser, torch.from_numpy(xT.reshape(shape).astype(np.float32)).to(dev), mu, s, xT


def _analytic_error(dev, respacing, sampler, order=2):
    den, xT_d, mu, s, xT = _analytic(dev)
    d = _diffusion(respacing)
    kw = dict(noise=xT_d, clip_denoised=False, model_kwargs={}, device=dev)
    out = d.ddim_sample_loop(den, tuple(xT_d.shape), **kw) if sampler == "ddim" else \
        d.dpm_solver_sample_loop(den, tuple(xT_d.shape), order=order, **kw)
    a2 = d.alphas_cumprod[-1]
    exact = mu + s * (xT - np.sqrt(a2) * mu) / np.sqrt(a2 * s ** 2 + (1.0 - a2))     # (x - a mu) / sqrt(a^2 s^2 + sigma^2) is constant
    got = out.double().cpu().numpy().reshape(-1)
    return float(np.linalg.norm(got - exact) / np.linalg.norm(exact)), out


def test_solver_order_on_the_analytic_problem(dev):
    e_ddim20, ddim20 = _analytic_error(dev, "ddim20", "ddim")
    e_ms20, _ = _analytic_error(dev, "ddim20", MS)
    e_ms40, _ = _analytic_error(dev, "ddim40", MS)
    e_ddim40, _ = _analytic_error(dev, "ddim40", "ddim")
    e_o1, o1 = _analytic_error(dev, "ddim20", MS, order=1)
    o1_vs_ddim = rel_l2(o1.cpu(), ddim20.cpu())
    record("multistep/analytic_gaussian", ddim20=e_ddim20, ddim40=e_ddim40, dpm2m_20=e_ms20, dpm2m_40=e_ms40, order1_20=e_o1,
           ddim20_over_2m20=e_ddim20 / e_ms20, ms20_over_ms40=e_ms20 / e_ms40, order1_vs_ddim_rel_l2=o1_vs_ddim)
    assert e_ms20 <= e_ddim20 / 5, (e_ms20, e_ddim20)                   # measured in float64: 4.4e-3 against 5.2e-2
    assert e_ms40 <= e_ms20 / 2.5, (e_ms40, e_ms20)                     # second order: ~4.4x per doubling (DDIM: 1.95x)
    assert o1_vs_ddim < 1e-5, o1_vs_ddim                               # order 1 is DDIM with eta = 0, to fp32 rounding


# ---------------------------------------------------------------------------------------------- 3. fused step and loop

@pytest.mark.parametrize("precision", PRECISIONS)
def test_fused_step_matches_the_restatement(dev, precision):
    model, diff = _models(dev, precision)["face"]
    B, Cf = 2, model.nfeats
    y = _y("face", model, B, T, dev)
    x = _randn(B, Cf, 1, T).to(dev)
    prev = _randn(B, Cf, 1, T, seed=SEED + 3, scale=0.8).to(dev)
    known = _randn(B, Cf, 1, T, seed=SEED + 2, scale=3.0).to(dev)
    cf, tmap = diff._multistep_coefs(dev), diff._timestep_map(dev)
    cf_h = cf.cpu().numpy()
    masks = {"none": None, **_masks(B, Cf, T)}
    for step in (7, 1, 0):
        t = torch.full((B,), step, dtype=torch.int64, device=dev)
        g = model(x, tmap[t], y).cpu().numpy().transpose(0, 2, 1)            # the guided forward [B, T, C] -> [B, C, T]
        for kind, m in masks.items():
            mask_u8 = None if m is None else expand_mask(m.to(dev), B, Cf, T)
            kn = None if m is None else known
            for clip in (False, True):
                for hist in (None, prev):
                    xn, x0 = model.a2p_sample_step_multistep(x, t, tmap, cf, y, hist, clip, kn, mask_u8)
                    w0 = np.clip(g, -1, 1).astype(np.float32) if clip else g.copy()
                    if m is not None:
                        w0 = np.where(mask_u8.squeeze(2).cpu().numpy().astype(bool), known.squeeze(2).cpu().numpy(), w0)
                    wn = _restated_update(x.squeeze(2).cpu().numpy(), w0, None if hist is None else hist.squeeze(2).cpu().numpy(), cf_h,
                                          step)
                    assert np.array_equal(x0.squeeze(2).cpu().numpy().view(np.int32), w0.view(np.int32)), (step, kind, clip)
                    assert np.array_equal(xn.squeeze(2).cpu().numpy().view(np.int32), wn.view(np.int32)), (step, kind, clip, hist is None)
                    if m is not None:                              # an all-false mask is the plain step
                        none = torch.zeros_like(mask_u8)
                        pn, p0 = model.a2p_sample_step_multistep(x, t, tmap, cf, y, hist, clip, known, none)
                        qn, q0 = model.a2p_sample_step_multistep(x, t, tmap, cf, y, hist, clip)
                        assert _bits_equal(pn, qn) and _bits_equal(p0, q0)
    with pytest.raises(_lib.A2PError, match="alias"):
        fm = model.model
        out = torch.empty_like(x)
        sc = y["scale"].float().contiguous()
        _lib.check(fm._lib().a2p_sample_step_multistep(fm._ctx, _lib.ptr(x), _lib.ptr(t), _lib.ptr(tmap), cf.shape[1], _lib.ptr(sc),
                                                       _lib.ptr(cf), _lib.ptr(prev), 0, None, None, _lib.ptr(out), _lib.ptr(prev),
                                                       _lib.current_stream(dev)), "a2p_sample_step_multistep")
    model.model.check_finite()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fused_loop_equals_the_generic_path(dev, precision):
    model, diff = _models(dev, precision)["face"]
    B, Cf = 2, model.nfeats
    y = _y("face", model, B, T, dev)
    xT = _randn(B, Cf, 1, T).to(dev)
    for order in (2, 1):
        fused = diff.dpm_solver_sample_loop(model, (B, Cf, 1, T), noise=xT, clip_denoised=False, model_kwargs={"y": y}, order=order)
        generic = diff.dpm_solver_sample_loop(lambda x, t, **kw: model(x, t, **kw), (B, Cf, 1, T), noise=xT, clip_denoised=False,
                                              model_kwargs={"y": y}, device=dev, order=order)
        assert torch.isfinite(fused).all() and _bits_equal(fused, generic), order
    model.model.check_finite()


def test_fp32_loop_against_the_float64_oracle(dev):
    """10 steps of 2M at face 2 layers, B=2, T=240, fp32, against the CPU oracle forward in float64 and the table restated in float64."""
    from oracle import a2p_oracle as O
    from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from audio2photoreal_amd.spec import face_spec
    from audio2photoreal_amd.synthetic import synthetic_inputs, synthetic_state_dict
    spec = face_spec(num_layers=2)
    sd = synthetic_state_dict(spec, SEED)
    B = 2
    inp = synthetic_inputs(spec, B, T, SEED)
    model, d = create_model_and_diffusion(default_args("face", layers=2, timestep_respacing="ddim10"), "test", precision="fp32", max_batch=B)
    load_model(model, sd)
    cfg = ClassifierFreeSampleModel(model.to(dev).eval())
    y = {"cond_embed": inp["cond_embed"].to(dev), "scale": torch.full((B,), 10.0, device=dev)}
    got = d.dpm_solver_sample_loop(cfg, (B, spec.nfeats, 1, T), noise=inp["x_T"].to(dev), clip_denoised=False, model_kwargs={"y": y}).cpu()
    model.release()

    den = O.OracleDenoiser(sd, "face", 2, spec.num_heads, dtype=torch.float64)
    tab = _restated(d)
    x, hist = inp["x_T"].double(), None
    for i in range(d.num_timesteps)[::-1]:
        ts = torch.full((B,), d.timestep_map[i], dtype=torch.int64)
        x0 = den.forward_cfg(x, ts, inp["cond_embed"].double(), torch.full((B,), 10.0)).permute(0, 2, 1).unsqueeze(2)
        cx, b1, b2, p2 = tab[:, i]
        x = x0 if i == 0 else (cx * x + b1 * x0 if hist is None else cx * x + b2 * x0 + p2 * hist)
        hist = x0
    err = rel_l2(got, x)
    record("multistep/oracle_face_L2_B2_T240_ddim10_fp32", rel_l2=err)
    assert err < 1e-3, err


def test_fp16_loop_against_fp32_at_the_headline_shape(dev):
    """20 steps of 2M at face B=8, T=600 (8 layers, synthetic weights): the fp16 result against the fp32 one."""
    from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from audio2photoreal_amd.spec import face_spec
    from audio2photoreal_amd.synthetic import synthetic_inputs, synthetic_state_dict
    spec = face_spec()
    sd = synthetic_state_dict(spec, SEED)
    B, Tl = 8, 600
    inp = synthetic_inputs(spec, B, Tl, SEED)
    out = {}
    for precision in ("fp32", "fp16"):
        model, d = create_model_and_diffusion(default_args("face", timestep_respacing="ddim20"), "test", precision=precision, max_batch=B)
        load_model(model, sd)
        cfg = ClassifierFreeSampleModel(model.to(dev).eval())
        y = {"cond_embed": inp["cond_embed"].to(dev), "scale": torch.full((B,), 10.0, device=dev)}
        out[precision] = d.dpm_solver_sample_loop(cfg, (B, spec.nfeats, 1, Tl), noise=inp["x_T"].to(dev), clip_denoised=False,
                                                  model_kwargs={"y": y}).cpu()
        assert model.escalated_from is None
        model.release()
    err = rel_l2(out["fp16"], out["fp32"])
    record("multistep/fp16_vs_fp32_face_B8_T600_ddim20", rel_l2=err)
    assert torch.isfinite(out["fp16"]).all() and err < 7.7e-4, err      # the 16-bit bar: min(1e-3, 2x the measured 3.85e-4)


# ---------------------------------------------------------------------------------------------- 4. held elements

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fmt", ["face", "pose"])
def test_held_elements_come_back_exactly(dev, fmt, precision):
    model, diff = _models(dev, precision)[fmt]
    B, Cf = 2, model.nfeats
    y = _y(fmt, model, B, T, dev)
    known = _randn(B, Cf, 1, T, seed=SEED + 2, scale=3.0).to(dev)
    xT = _randn(B, Cf, 1, T).to(dev)
    for kind, m in _masks(B, Cf, T).items():
        out = inpaint_sample_loop(diff, model, y, known, m.to(dev), xT, sampler=MS)
        held = expand_mask(m.to(dev), B, Cf, T).bool()
        assert torch.isfinite(out).all() and _bits_equal(out[held], known[held]), kind
    none = torch.zeros(B, T, dtype=torch.bool, device=dev)
    plain = diff.dpm_solver_sample_loop(model, (B, Cf, 1, T), noise=xT, clip_denoised=False, model_kwargs={"y": y})
    assert _bits_equal(inpaint_sample_loop(diff, model, y, known, none, xT, sampler=MS), plain)


def test_continue_recording_holds_the_previous_frames(dev, monkeypatch):
    ms = _models(dev, "fp16")
    face, pose = ms["face"], ms["pose"]
    stats = _stats()
    first = generate_from_recording(face, pose, stats, _recording(8.2), SR, num_repetitions=2, seed=SEED, sampler=MS)
    assert first["T"] == 240 and all(np.isfinite(first[k]).all() for k in ("face", "pose"))
    ddim = generate_from_recording(face, pose, stats, _recording(8.2), SR, num_repetitions=2, seed=SEED)
    assert not np.array_equal(first["face"], ddim["face"])          # the sampler reached the loops
    calls = []
    loop = inpaint.inpaint_sample_loop

    def spy(diffusion, model, y, known, known_mask, noise, **kw):
        out = loop(diffusion, model, y, known, known_mask, noise, **kw)
        calls.append((model.nfeats, kw.get("sampler"), out.cpu()))
        return out
    monkeypatch.setattr(inpaint, "inpaint_sample_loop", spy)
    out = continue_recording(face, pose, stats, _recording(4.2, seed=8), SR, first, context_frames=120, seed=SEED, sampler=MS)
    assert out["T"] == 120 and all(np.isfinite(out[k]).all() for k in ("face", "pose", "keyframes"))
    assert sorted((c[0], c[1]) for c in calls) == [(104, MS), (256, MS)]
    for nf, _, window in calls:
        mean, std, prev = ((stats["code_mean"], stats["code_std"], first["face"]) if nf == 256 else
                           (stats["pose_mean"], stats["pose_std"], first["pose"]))
        assert torch.equal(window[:, :, 0, :120], _norm(prev[:, -120:], mean, std))


# ---------------------------------------------------------------------------------------------- 5. windows

@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_window_is_the_plain_loop(dev, precision):
    model, diff = _models(dev, precision)["face"]
    B, Cf = 2, model.nfeats
    y = _y("face", model, B, T, dev)
    xT = _randn(B, Cf, 1, T).to(dev)
    plan = plan_windows(T, T_w=T)
    assert plan.W == 1
    win = windowed_sample_loop(diff, model, plan, B, y, xT, sampler=MS)
    plain = diff.dpm_solver_sample_loop(model, (B, Cf, 1, T), noise=xT, clip_denoised=False, model_kwargs={"y": y})
    assert torch.isfinite(plain).all() and _bits_equal(win, plain)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_window_copies_stay_identical(dev, precision):
    """R=2 x W=3 windows of 240 frames over 480: after every step every window copy of a global frame holds the global result's
    bits, for the state and for pred_xstart (the next step's history)."""
    model, diff = _models(dev, precision)["face"]
    plan = plan_windows(480, T_w=T, min_overlap=120)
    R, Cf = 2, model.nfeats
    assert plan.W == 3 and plan.starts == [0, 120, 240]
    y = _y("face", model, R * plan.W, T, dev)
    cf, tmap = diff._multistep_coefs(dev), diff._timestep_map(dev)
    from audio2photoreal_amd.sample.long_form import _starts_host
    starts, weights = _starts_host(plan), torch.from_numpy(plan.weights).to(dev).contiguous()
    xg = _randn(R, Cf, 1, plan.T_total).to(dev)
    x = window_gather(xg, plan, channels_first=True)
    hist = None
    for step in range(diff.num_timesteps)[::-1]:
        t = torch.full((R * plan.W,), step, dtype=torch.int64, device=dev)
        x, x0, xg, x0g = model.a2p_sample_step_windowed_multistep(x, t, tmap, cf, y, hist, False, starts, weights, plan.T_total)
        assert _bits_equal(x, window_gather(xg, plan, channels_first=True)), step
        assert _bits_equal(x0, window_gather(x0g, plan, channels_first=True)), step
        hist = x0
    assert torch.isfinite(xg).all() and _bits_equal(xg, x0g)        # the last step returns pred_xstart
    model.model.check_finite()


def test_long_recording_with_the_solver(dev):
    ms = _models(dev, "fp16")
    face, pose = ms["face"], ms["pose"]
    out = generate_from_long_recording(face, pose, _stats(), _recording(31.0), SR, num_repetitions=2, seed=SEED, sampler=MS)
    Tn = out["T"]
    assert Tn == 840 and len(out["window_starts"]) == 2                # 28 s of whole 4 s blocks, two windows of 600 frames
    assert out["face"].shape == (2, Tn, 256) and out["pose"].shape == (2, Tn, 104)
    assert all(np.isfinite(out[k]).all() for k in ("face", "pose", "keyframes"))
    assert face[0].a2p_check_finite() is None and pose[0].a2p_check_finite() is None


# ---------------------------------------------------------------------------------------------- 6. escalation

def _loop_plain(diffusion, cfg, spec, d, B=2, T=240):
    from test_envelope_hip import SEED as ESEED, _face_y
    from audio2photoreal_amd.synthetic import synthetic_tensor
    return diffusion.dpm_solver_sample_loop(cfg, (B, spec.nfeats, 1, T), clip_denoised=False, model_kwargs={"y": _face_y(B, T, d)},
                                            noise=synthetic_tensor(ESEED, "x_T", (B, spec.nfeats, 1, T)).to(d))


def _loop_held(diffusion, cfg, spec, d, B=2, T=240):
    from test_envelope_hip import SEED as ESEED, _face_y
    from audio2photoreal_amd.synthetic import synthetic_tensor
    known = synthetic_tensor(ESEED, "known", (B, spec.nfeats, 1, T)).to(d)
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask[:, :60] = True
    mask[1, 200:] = True
    return inpaint_sample_loop(diffusion, cfg, _face_y(B, T, d), known, mask.to(d),
                               synthetic_tensor(ESEED, "x_T", (B, spec.nfeats, 1, T)).to(d), sampler=MS)


def _loop_windowed(diffusion, cfg, spec, d, B=2, T=240):
    from test_envelope_hip import SEED as ESEED, _face_y
    from audio2photoreal_amd.synthetic import synthetic_tensor
    plan = plan_windows(360, T_w=T)
    assert plan.W == B == 2, plan
    return windowed_sample_loop(diffusion, cfg, plan, 1, _face_y(B, T, d), synthetic_tensor(ESEED, "x_T", (1, spec.nfeats, 1, 360)).to(d),
                                sampler=MS)


@pytest.mark.parametrize("loop", ["plain", "held", "windowed"])
def test_escalated_fp16_multistep_loop_returns_the_fp32_bits(dev, loop):
    """As test_envelope_hip.test_escalated_fp16_loop_returns_the_fp32_bits for the 2M loops: the first step is repeated on fp32 with
    the same (absent) history, and the result is a fresh fp32 model's, bit for bit."""
    from test_envelope_hip import _escalation_pair
    run = {"plain": _loop_plain, "held": _loop_held, "windowed": _loop_windowed}[loop]
    out = _escalation_pair(dev, 2, "ddim5", run)
    e, f = out["fp16"], out["fp32"]
    equal = torch.equal(e["out"], f["out"])
    record(f"multistep/escalation_face_B2_T240/{loop}", equal=equal, max_abs_diff=float((e["out"] - f["out"]).abs().max()),
           warnings=e["warnings"], precision_after=e["precision_after"], escalated_from=e["escalated_from"])
    assert e["precision_after"] == "fp32" and e["escalated_from"] == "fp16" and e["warnings"] == 1, e
    assert f["warnings"] == 0 and f["escalated_from"] is None, f
    assert torch.isfinite(f["out"]).all() and equal


# ---------------------------------------------------------------------------------------------- 7. measured only

def test_measure_20_steps_against_ddim1000(dev):
    """No assertion on the distances: the synthetic 2-layer model is not a trained denoiser, so these say nothing about quality."""
    model, _ = _models(dev, "fp32")["face"]
    B, Cf = 2, model.nfeats
    y = _y("face", model, B, T, dev)
    xT = _randn(B, Cf, 1, T).to(dev)
    kw = dict(noise=xT, clip_denoised=False, model_kwargs={"y": y})
    ref = _diffusion("").ddim_sample_loop(model, (B, Cf, 1, T), **kw)
    ms20 = _diffusion("ddim20").dpm_solver_sample_loop(model, (B, Cf, 1, T), **kw)
    dd20 = _diffusion("ddim20").ddim_sample_loop(model, (B, Cf, 1, T), **kw)
    record("multistep/synthetic_face_L2_B2_T240_vs_ddim1000", dpm2m_20=rel_l2(ms20.cpu(), ref.cpu()), ddim_20=rel_l2(dd20.cpu(), ref.cpu()))
    assert all(torch.isfinite(v).all() for v in (ref, ms20, dd20))
