"""What a chain forward launches, restated from the dispatch rules of csrc/a2p_lib_run.h as they stood BEFORE there was one
plan (run_forward, forward_body, decoder_layer_chain, chain_pick_nw, chain_pick_family, chain4_wanted, chain4_final_ok,
chain4_pick_mt, chain_in_wanted and the candidate loop / mix rule of launch_chain), and the cases of tests/test_chain_plan_hip.py.
Test infrastructure: pure Python, no GPU, no library.

`expected(case)` gives the workgroup shape, the family pair and one record per chain launch in launch order, in the layout of
a2p_debug_read "chain_picks": (family, d, mt, nw, mode, variant, grid, block, n_tall, stream).  `counters(picks)` and
`class_counts(picks)` derive what the long-standing names must show for the same forward: the *_launches counters and the launch
count of each KERNEL_CHAIN_* timing class."""
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

PRE, MID, POST, MIDPOST, IN = 0, 1, 2, 3, 4                       # CHAIN_* of csrc/kernels_chain.h
UNIFORM, MIX, NEXT, LAST, LAST_FINAL, PAIRED_TAIL = range(6)      # variant: generation 1 (0, 1) | tall (2 ..)
S_GEN1, S_TALL, S_TALL_WIDE, S_IN = range(4)                      # which packed weight stream the kernel reads
FIELDS = ("family", "d", "mt", "nw", "mode", "variant", "grid", "block", "n_tall", "stream")
MAX_PICKS = 64
CUS = 256

# the models of audio2photoreal_amd/spec.py: d_model, feature channels, decoder layers, head_dim, keyframe step
MODELS = {"face": dict(d=512, C=256, L=8, dh=64, pose=False), "pose": dict(d=256, C=104, L=6, dh=32, pose=True)}
SWITCHES = ("A2P_CHAIN_V", "A2P_CHAIN_ROWS", "A2P_CHAIN_NW", "A2P_CHAIN_MT", "A2P_CHAIN_NO_MIX", "A2P_NO_SHARED_HALF", "A2P_NO_FUSED_IN",
            "A2P_NO_FUSED_FINAL", "A2P_NO_FUSED_KF", "A2P_FUSED_TAIL", "A2P_NO_CHAIN", "A2P_NO_SMALL")


@dataclass(frozen=True)
class Case:
    name: str
    fmt: str                                   # "face" | "pose"
    B: int
    T: int
    guided: bool                               # classifier-free guidance: 2B sequences in one pass
    env: Tuple[Tuple[str, str], ...] = ()      # switches a context re-reads (audio2photoreal_amd/_lib.py ENV_SWITCHES)
    ddpm_step: bool = False                    # a guided a2p_sample_step with the DDPM sampler instead of a plain forward
    tail16: bool = False                       # the context is created under A2P_TAIL16=1
    layers: Optional[int] = None               # decoder layers of a shallow synthetic model; None: the model's own depth
    hits: Tuple[Tuple[int, ...], ...] = ()     # SHALLOW_CASES: the kChainInst key every launch must hit, in launch order

    @property
    def switches(self) -> Dict[str, str]:
        return dict(self.env)


def _e(**kw):
    return tuple(sorted(("A2P_" + k, str(v)) for k, v in kw.items()))


FACE80 = dict(fmt="face", B=1, T=80)
CASES = (
    Case("c01_face_unguided", guided=False, env=_e(CHAIN_V=4, CHAIN_ROWS=1), **FACE80),
    Case("c02_face_guided", guided=True, env=_e(CHAIN_V=4, CHAIN_ROWS=1), **FACE80),
    Case("c03_no_shared_half", guided=True, env=_e(CHAIN_V=4, CHAIN_ROWS=1, NO_SHARED_HALF=1), **FACE80),
    Case("c03_no_fused_in", guided=True, env=_e(CHAIN_V=4, CHAIN_ROWS=1, NO_FUSED_IN=1), **FACE80),
    Case("c03_no_fused_final", guided=True, env=_e(CHAIN_V=4, CHAIN_ROWS=1, NO_FUSED_FINAL=1), **FACE80),
    Case("c04_T72", "face", 1, 72, True, _e(CHAIN_V=4, CHAIN_ROWS=1)),
    Case("c04_T84", "face", 1, 84, True, _e(CHAIN_V=4, CHAIN_ROWS=1)),
    Case("c05_ddpm_paired", "face", 1, 96, True, _e(CHAIN_V=4, CHAIN_ROWS=1), ddpm_step=True),
    Case("c06_ddpm_tail_behind", "face", 1, 96, True, _e(CHAIN_V=4, CHAIN_ROWS=1, FUSED_TAIL=0), ddpm_step=True),
    Case("c07_gen1_nw8", guided=True, env=_e(CHAIN_V=1, CHAIN_ROWS=1), **FACE80),
    Case("c07_gen1_nw4", guided=True, env=_e(CHAIN_V=1, CHAIN_ROWS=1, CHAIN_NW=4), **FACE80),
    Case("c07_family41", guided=True, env=_e(CHAIN_V=41, CHAIN_ROWS=1), **FACE80),
    # forced heights, in both families: MT=5 with the tall kernels away is a height the 8-wave generation-1 kernels do not have
    *(Case(f"c08_mt{mt}_v{v}", guided=True, env=_e(CHAIN_V=v, CHAIN_MT=mt), **FACE80) for mt in (2, 4, 5) for v in (4, 1)),
    # 12480 rows: the candidate loop takes 32-row panels there (2 rounds x 24 against 2 x 28), so both launches are uniform ...
    Case("c09_B13_T480", "face", 13, 480, True, _e(CHAIN_V=1)),
    Case("c10_B13_T480_no_mix", "face", 13, 480, True, _e(CHAIN_V=1, CHAIN_NO_MIX=1)),
    # ... the smallest guided batch of 480-frame clips whose MID and POST launches mix panel heights is 24960 rows (520 panels of 48:
    # W=512, n_tall=24); without the shared half the PRE launch mixes too
    Case("c09_B26_T480_mix", "face", 26, 480, True, _e(CHAIN_V=1)),
    Case("c09_B26_T480_mix_pre", "face", 26, 480, True, _e(CHAIN_V=1, NO_SHARED_HALF=1)),
    Case("c10_B26_T480_no_mix", "face", 26, 480, True, _e(CHAIN_V=1, CHAIN_NO_MIX=1)),
    Case("c11_tail16", guided=True, env=_e(CHAIN_V=4, CHAIN_ROWS=1), tail16=True, **FACE80),
    Case("c12_body_midpost", "pose", 1, 80, True, _e(CHAIN_V=4, CHAIN_ROWS=1)),
    Case("c13_body_no_fused_kf", "pose", 1, 80, True, _e(CHAIN_V=4, CHAIN_ROWS=1, NO_FUSED_KF=1)),
    Case("c14_body_nw4_mt6", "pose", 1, 80, True, _e(CHAIN_V=4, CHAIN_NW=4, CHAIN_MT=6)),
)
BY_NAME = {c.name: c for c in CASES}

# Every kChainInst key (family, d, mt, nw, mode, variant) of csrc/a2p_lib_run.h, written out by hand in the table's order
# (tests/test_forward_paths_cpu.py compares it with the CI(...) lines of the source).
_G8_512 = tuple((1, 512, mt, 8, mode, UNIFORM) for mt in (2, 3, 4) for mode in (PRE, MID, POST))
_G8_MIX = ((1, 512, 3, 8, PRE, MIX), (1, 512, 3, 8, MID, MIX), (1, 512, 3, 8, POST, MIX))
_G8_256 = tuple((1, 256, mt, 8, mode, UNIFORM) for mt in (2, 3, 4, 5) for mode in (PRE, MID, POST))
_G4_512 = tuple((1, 512, mt, 4, mode, UNIFORM) for mt in (2, 3, 4) for mode in (PRE, MID, POST))
_G4_256 = tuple((1, 256, mt, 4, mode, UNIFORM) for mt in (2, 3, 4, 5, 6) for mode in (PRE, MID, POST))
_MIDPOST = tuple((1, 256, mt, 8, MIDPOST, UNIFORM) for mt in (2, 3, 4, 5)) + tuple((1, 256, mt, 4, MIDPOST, UNIFORM) for mt in (2, 3, 4, 5, 6))
_TALL = ((4, 512, 3, 8, IN, NEXT), (4, 512, 3, 8, MID, NEXT), (4, 512, 3, 8, POST, NEXT), (4, 512, 3, 8, POST, LAST), (4, 512, 3, 8, POST, LAST_FINAL),
         (4, 512, 3, 8, POST, PAIRED_TAIL),
         (4, 512, 4, 8, IN, NEXT), (4, 512, 4, 8, MID, NEXT), (4, 512, 4, 8, POST, NEXT), (4, 512, 4, 8, POST, LAST), (4, 512, 4, 8, POST, LAST_FINAL),
         (4, 512, 5, 8, IN, NEXT), (4, 512, 5, 8, MID, NEXT), (4, 512, 5, 8, POST, NEXT), (4, 512, 5, 8, POST, LAST), (4, 512, 5, 8, POST, LAST_FINAL))
INSTANCES = _G8_512 + _G8_MIX + _G8_256 + _G4_512 + _G4_256 + _MIDPOST + _TALL

# ---- shallow synthetic models (1 and 2 decoder layers): the cases of tests/test_forward_paths_hip.py.  Shapes (B, T), all guided unless said:
#   S88  2 x 88: 352 rows; 88 is a multiple of 8 and >= 80 (the tall contract) and no multiple of 32 / 48 / 64 / 80 / 96 -- every panel height has a
#        ragged last panel and panels that straddle sequences
#   S50  3 x 50: T is no multiple of 4 (V^T 4-row groups straddle sequences), odd batch; generation 1 only
#   S17  5 x 17 (body): T >= 16 is the MIDPOST contract; at 17 every 16-row tile straddles two key sets; one keyframe token
#   SMIX 26 x 480 (face, one layer): the smallest batch of 480-frame clips whose launches mix 64- and 48-row panels
# `hits` is written from the launch pattern of the path, NOT from expected(): the CPU test holds the two against each other.
S88, S50, S17, SMIX, S96 = (2, 88), (3, 50), (5, 17), (26, 480), (2, 96)
GEN1_HEIGHTS = {"face": tuple((mt, nw) for nw in (8, 4) for mt in (2, 3, 4)),
                "pose": tuple((mt, 8) for mt in (2, 3, 4, 5)) + tuple((mt, 4) for mt in (2, 3, 4, 5, 6))}


def _shallow(name, fmt, shape, hits, layers=2, guided=True, **kw):
    flags = {k: kw.pop(k) for k in ("ddpm_step", "tail16") if k in kw}
    return Case(name, fmt, shape[0], shape[1], guided, _e(**kw), layers=layers, hits=tuple(hits), **flags)


def _gen1_hits(d, mt, nw, layers, kind="post", variant=UNIFORM, pre=None):
    """PRE once, then per layer MID + POST (face), MID + MIDPOST (body) or MID + MID2 + POST (body without the fused keyframe attention)."""
    per_layer = {"post": (MID, POST), "midpost": (MID, MIDPOST), "mid2": (MID, MID, POST)}[kind]
    return [pre or (1, d, mt, nw, PRE, variant)] + [(1, d, mt, nw, mode, variant) for _ in range(layers) for mode in per_layer]


def _tall_hits(mt, first, last, post0=None):
    """Two layers of the tall family: `first` = layer 0's first kernel, `post0` = layer 0's POST kernel where it is not tall, `last` = the last POST variant."""
    return [first, (4, 512, mt, 8, MID, NEXT), post0 or (4, 512, mt, 8, POST, NEXT), (4, 512, mt, 8, MID, NEXT), (4, 512, mt, 8, POST, last)]


def _shallow_cases():
    out = []
    for sname, shape in (("S88", S88), ("S50", S50)):
        for mt, nw in GEN1_HEIGHTS["face"]:
            out.append(_shallow(f"face_{sname}_gen1_mt{mt}_nw{nw}", "face", shape, _gen1_hits(512, mt, nw, 2), CHAIN_V=1, CHAIN_MT=mt, CHAIN_NW=nw))
        for mt, nw in GEN1_HEIGHTS["pose"]:
            out.append(_shallow(f"pose_{sname}_midpost_mt{mt}_nw{nw}", "pose", shape, _gen1_hits(256, mt, nw, 2, "midpost"), CHAIN_MT=mt, CHAIN_NW=nw))
            out.append(_shallow(f"pose_{sname}_no_fused_kf_mt{mt}_nw{nw}", "pose", shape, _gen1_hits(256, mt, nw, 2, "mid2"),
                                CHAIN_MT=mt, CHAIN_NW=nw, NO_FUSED_KF=1))
    for mt, nw in GEN1_HEIGHTS["pose"]:
        out.append(_shallow(f"pose_S17_midpost_mt{mt}_nw{nw}", "pose", S17, _gen1_hits(256, mt, nw, 2, "midpost"), CHAIN_MT=mt, CHAIN_NW=nw))
    for mt in (3, 4, 5):
        tall_in = (4, 512, mt, 8, IN, NEXT)
        # a generation-1 kernel of a forward whose forced height it does not have (80 rows) takes the candidate loop: 32-row panels at 176 and 352 rows
        # (6 / 11 panels: one round of 24 against one of 28 for 48-row panels)
        g1 = mt if mt <= 4 else 2
        env = dict(CHAIN_V=4, CHAIN_MT=mt)
        out.append(_shallow(f"face_S88_tall_mt{mt}", "face", S88, _tall_hits(mt, tall_in, LAST_FINAL), **env))
        out.append(_shallow(f"face_S88_tall_mt{mt}_no_fused_final", "face", S88, _tall_hits(mt, tall_in, LAST), NO_FUSED_FINAL=1, **env))
        out.append(_shallow(f"face_S88_tall_mt{mt}_no_fused_in", "face", S88, _tall_hits(mt, (1, 512, g1, 8, PRE, UNIFORM), LAST_FINAL), NO_FUSED_IN=1, **env))
        out.append(_shallow(f"face_S88_tall_mt{mt}_no_shared_half", "face", S88, _tall_hits(mt, (1, 512, g1, 8, PRE, UNIFORM), LAST_FINAL),
                            NO_SHARED_HALF=1, **env))
        out.append(_shallow(f"face_S88_tall_mt{mt}_family41", "face", S88, _tall_hits(mt, tall_in, LAST_FINAL, post0=(1, 512, g1, 8, POST, UNIFORM)),
                            CHAIN_V=41, CHAIN_MT=mt))
        out.append(_shallow(f"face_S88_tall_mt{mt}_unguided", "face", S88, _tall_hits(mt, tall_in, LAST_FINAL), guided=False, **env))
    # A2P_TAIL16: final_layer on 16-bit operands inside the last generation-1 POST kernel; no split-operand islands, so no fused input kernel either
    out.append(_shallow("face_S88_tail16_gen1", "face", S88, _gen1_hits(512, 3, 8, 2), tail16=True, CHAIN_V=1, CHAIN_MT=3, CHAIN_NW=8))
    out.append(_shallow("face_S88_tail16_tall", "face", S88,
                        [(1, 512, 3, 8, PRE, UNIFORM), (4, 512, 3, 8, MID, NEXT), (4, 512, 3, 8, POST, NEXT), (4, 512, 3, 8, MID, NEXT), (1, 512, 3, 8, POST, UNIFORM)],
                        tail16=True, CHAIN_V=4, CHAIN_MT=3))
    # one guided DDPM step: paired 48-row panels and the step tail in the last POST kernel (384 rows: 48-row panels by the cost rule)
    out.append(_shallow("face_S96_ddpm_paired_tail", "face", S96, _tall_hits(3, (4, 512, 3, 8, IN, NEXT), PAIRED_TAIL), ddpm_step=True, CHAIN_V=4, CHAIN_ROWS=1))
    # one layer, 24960 rows: MID and POST mix panel heights (the shared first half, 12480 rows, takes 32-row panels); without the shared half PRE mixes too
    out.append(_shallow("face_SMIX", "face", SMIX, _gen1_hits(512, 3, 8, 1, variant=MIX, pre=(1, 512, 2, 8, PRE, UNIFORM)), layers=1, CHAIN_V=1))
    out.append(_shallow("face_SMIX_no_shared_half", "face", SMIX, _gen1_hits(512, 3, 8, 1, variant=MIX), layers=1, CHAIN_V=1, NO_SHARED_HALF=1))
    return tuple(out)


SHALLOW_CASES = _shallow_cases()
SHALLOW_BY_NAME = {c.name: c for c in SHALLOW_CASES}
# instances no shallow case launches: {key: the reason, naming the source line that makes it unreachable}.  At most 4 entries.
NOT_REACHED: Dict[Tuple[int, ...], str] = {}


def _num(sw, name, default=0):
    return int(sw[name]) if sw.get(name) not in (None, "") else default


def _flag(sw, name):
    return sw.get(name) not in (None, "", "0")


def pick_nw(case: Case) -> int:
    """chain_pick_nw: 8 waves by rule; 4 for forced panel heights only the 4-wave kernels have."""
    sw, m = case.switches, MODELS[case.fmt]
    nw, mt = _num(sw, "A2P_CHAIN_NW"), _num(sw, "A2P_CHAIN_MT")
    if nw:
        return 8 if nw == 8 else 4
    if mt == 5 and m["d"] == 512 and _num(sw, "A2P_CHAIN_V") != 1 and not m["pose"]:
        return 8
    return 4 if (mt and ((mt > 4 and m["d"] == 512) or mt > 5)) else 8


def pick_family(case: Case, nw: int):
    """chain_pick_family where the switch forces it: (MID, POST) or None (measured in situ)."""
    v, m = _num(case.switches, "A2P_CHAIN_V"), MODELS[case.fmt]
    if v == 1 or m["pose"] or m["d"] != 512 or nw != 8:
        return (1, 1)
    return {4: (4, 4), 41: (4, 1)}.get(v)


def takes_chain_path(case: Case) -> bool:
    """run_forward: the chain kernels from the row threshold on (1100 rows against the small-forward kernels of the face model, 960
    otherwise), or whenever a panel height is forced."""
    sw, m = case.switches, MODELS[case.fmt]
    rows = (2 if case.guided else 1) * case.B * case.T
    thr = _num(sw, "A2P_CHAIN_ROWS", 1100)
    if m["pose"]:
        thr = min(thr, 960)
    return rows >= thr or _num(sw, "A2P_CHAIN_MT") != 0


def _rounds_cost(M, mt):
    blocks = -(-M // (16 * mt))
    return -(-blocks // CUS) * (16 + 4 * mt)


def _tall_mt(sw, M):
    mt = _num(sw, "A2P_CHAIN_MT")
    if 3 <= mt <= 5:
        return mt
    return min((3, 4, 5), key=lambda m: (_rounds_cost(M, m), m))          # fewest rounds, then the shorter panel


def _gen1(case, nw, mode, M):
    sw, d = case.switches, MODELS[case.fmt]["d"]
    forced = _num(sw, "A2P_CHAIN_MT")
    cands = {(512, 8): (4, 3, 2), (512, 4): (4, 3, 2), (256, 8): (5, 4, 3, 2), (256, 4): (6, 5, 4, 3, 2)}[(d, nw)]
    mt = forced
    if mt not in cands:
        free = [m for m in cands if not (d == 512 and m == 4)]               # d = 512: 64-row panels only when forced
        mt = min(free, key=lambda m: (_rounds_cost(M, m), free.index(m)))    # the first of equal costs: the taller panel
    grid = -(-M // (16 * mt))
    if nw == 8 and d == 512 and mt == 3 and not forced and grid > CUS and grid % CUS and not _flag(sw, "A2P_CHAIN_NO_MIX"):
        W = CUS * (-(-grid // CUS) - 1)
        n_tall = (M - 48 * W + 15) // 16
        if 0 < n_tall <= W:
            return (1, d, 3, nw, mode, MIX, W, 64 * nw, n_tall, S_GEN1)
    return (1, d, mt, nw, mode, UNIFORM, grid, 64 * nw, 0, S_GEN1)


def expected(case: Case, family=None):
    """{"nw", "family" (10 x MID + POST), "picks"} of one forward (or guided DDPM step) of the case.  `family`: the pair of a forward
    whose family the library measures (A2P_CHAIN_V unset)."""
    assert takes_chain_path(case), case
    sw, m = case.switches, MODELS[case.fmt]
    d, L, T, B = m["d"], case.layers or m["L"], case.T, case.B
    N = 2 * B if case.guided else B
    nw = pick_nw(case)
    fam = pick_family(case, nw) or family
    assert fam is not None, "a measured family has to be given"
    v = _num(sw, "A2P_CHAIN_V")
    face = not m["pose"] and d == 512
    islands = not case.tail16                                                # split-operand islands: the default of the 16-bit modes
    frames_ok = T % 8 == 0 and T >= 80
    shared_half = N == 2 * B and not _flag(sw, "A2P_NO_SHARED_HALF")
    fuse_in = (face and islands and m["C"] == 256 and v != 1 and not _flag(sw, "A2P_NO_FUSED_IN") and nw == 8 and frames_ok
               and (N == B or shared_half))
    fuse_final16 = not m["pose"] and case.tail16
    n_key = -(-T // 30)                                                      # keyframe tokens (keyframe_step 30)
    fuse_kf = m["pose"] and d == 256 and m["dh"] == 32 and T >= 16 and 1 <= n_key <= 32 and not _flag(sw, "A2P_NO_FUSED_KF")

    def tall(mode, M, last):
        """(family 4 record or None): the contract of the tall kernels, then the family of this chain -- except that a last POST kernel
        that can take final_layer in is tall whatever the family."""
        if not (face and v != 1 and nw == 8 and frames_ok) or (mode == POST and last and fuse_final16):
            return None                                                      # (final_layer on 16-bit operands rides on a generation-1 kernel)
        final_ok = mode == POST and last and islands and m["C"] == 256 and not _flag(sw, "A2P_NO_FUSED_FINAL")
        if not (final_ok or (fam[0] if mode == MID else fam[1]) == 4):
            return None
        mt = _tall_mt(sw, M)
        grid = -(-M // (16 * mt))
        variant = NEXT if (mode == MID or not last) else (LAST_FINAL if final_ok else LAST)
        if (variant == LAST_FINAL and case.ddpm_step and case.guided and _num(sw, "A2P_FUSED_TAIL", 1) and m["C"] == 256 and mt == 3):
            variant, grid = PAIRED_TAIL, B * (-(-T // 24))
        return (4, d, mt, 8, mode, variant, grid, 512, 0, S_TALL_WIDE if (mode == POST and mt <= 4) else S_TALL)

    picks = []
    for l in range(L):
        last = l + 1 == L
        if l == 0:
            M0 = (N // 2 if shared_half else N) * T
            if fuse_in:
                mt = _tall_mt(sw, M0)
                picks.append((4, d, mt, 8, IN, NEXT, -(-M0 // (16 * mt)), 512, 0, S_IN))
            else:
                picks.append(_gen1(case, nw, PRE, M0))
        picks.append(tall(MID, N * T, last) or _gen1(case, nw, MID, N * T))
        if m["pose"] and not fuse_kf:
            picks.append(_gen1(case, nw, MID, N * T))                        # MID2: the kernel in front of the keyframe attention
        if fuse_kf:
            picks.append(_gen1(case, nw, MIDPOST, N * T))
        else:
            picks.append(tall(POST, N * T, last) or _gen1(case, nw, POST, N * T))
    return {"nw": nw, "family": 10 * fam[0] + fam[1], "picks": picks}


def counters(picks) -> Dict[str, int]:
    """The a2p_debug_read counters one forward adds."""
    f = {k: i for i, k in enumerate(FIELDS)}
    return {"chain4_launches": sum(p[f["family"]] == 4 for p in picks),
            "chain_in_launches": sum(p[f["mode"]] == IN for p in picks),
            "final_fused_launches": sum(p[f["variant"]] in (LAST_FINAL, PAIRED_TAIL) for p in picks),
            "fused_tail_launches": sum(p[f["variant"]] == PAIRED_TAIL for p in picks)}


def class_counts(picks) -> Dict[str, int]:
    """Launches per timing class (a2p_kernel_timing): CHAIN_IN counts as the PRE work it contains."""
    mode = [p[FIELDS.index("mode")] for p in picks]
    return {"PRE": mode.count(PRE) + mode.count(IN), "MID": mode.count(MID), "POST": mode.count(POST), "MIDPOST": mode.count(MIDPOST)}
