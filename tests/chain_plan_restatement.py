"""What a chain forward launches, restated from the dispatch rules of csrc/a2p_lib_run.h as they stood BEFORE there was one
plan (run_forward, forward_body, decoder_layer_chain, chain_pick_nw, chain_pick_family, chain4_wanted, chain4_final_ok,
chain4_pick_mt, chain_in_wanted and the candidate loop / mix rule of launch_chain), and the cases of tests/test_chain_plan_hip.py.
Test infrastructure: pure Python, no GPU, no library.

`expected(case)` gives the workgroup shape, the family pair and one record per chain launch in launch order, in the layout of
a2p_debug_read "chain_picks": (family, d, mt, nw, mode, variant, grid, block, n_tall, stream).  `counters(picks)` and
`class_counts(picks)` derive what the long-standing names must show for the same forward: the *_launches counters and the launch
count of each KERNEL_CHAIN_* timing class."""
from dataclasses import dataclass
from typing import Dict, Tuple

PRE, MID, POST, MIDPOST, IN = 0, 1, 2, 3, 4                       # CHAIN_* of csrc/kernels_chain.h
UNIFORM, MIX, NEXT, LAST, LAST_FINAL, PAIRED_TAIL = range(6)      # variant: generation 1 (0, 1) | tall (2 ..)
S_GEN1, S_TALL, S_TALL_WIDE, S_IN = range(4)                      # which packed weight stream the kernel reads
FIELDS = ("family", "d", "mt", "nw", "mode", "variant", "grid", "block", "n_tall", "stream")
MAX_PICKS = 64
CUS = 256

# the models of audio2photoreal_amd/spec.py: d_model, feature channels, decoder layers, head_dim, keyframe step
MODELS = {"face": dict(d=512, C=256, L=8, dh=64, pose=False), "pose": dict(d=256, C=104, L=6, dh=32, pose=True)}
SWITCHES = ("A2P_CHAIN_V", "A2P_CHAIN_ROWS", "A2P_CHAIN_NW", "A2P_CHAIN_MT", "A2P_CHAIN_NO_MIX", "A2P_NO_SHARED_HALF", "A2P_NO_FUSED_IN",
            "A2P_NO_FUSED_FINAL", "A2P_NO_FUSED_KF", "A2P_FUSED_TAIL")


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
    d, L, T, B = m["d"], m["L"], case.T, case.B
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
