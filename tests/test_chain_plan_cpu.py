"""The cases of tests/chain_plan_restatement.py against the restated rule itself, without a launch: every branch of the chain
dispatch that tests/test_chain_plan_hip.py lists a case for is reached by that case, and every case takes the chain path."""
import chain_plan_restatement as R


def test_cases_reach_the_branches_they_are_for():
    """The restated rule on the cases themselves (no launch): every branch the cases are listed for is there."""
    f = {k: i for i, k in enumerate(R.FIELDS)}
    picks = {c.name: R.expected(c, family=(4, 4))["picks"] for c in R.CASES}

    def has(name, **kw):
        return any(all(p[f[k]] == v for k, v in kw.items()) for p in picks[name])

    assert has("c01_face_unguided", mode=R.IN, grid=2) and has("c01_face_unguided", mode=R.POST, variant=R.LAST_FINAL)
    assert has("c02_face_guided", mode=R.IN, grid=2) and has("c02_face_guided", mode=R.MID, family=4, grid=4)      # layer 0 on N/2 rows
    assert has("c03_no_shared_half", mode=R.PRE, family=1, grid=5) and has("c03_no_fused_in", mode=R.PRE, family=1, grid=3)
    assert has("c03_no_fused_final", variant=R.LAST) and not has("c03_no_fused_final", variant=R.LAST_FINAL)
    assert all(p[f["family"]] == 1 for n in ("c04_T72", "c04_T84") for p in picks[n])
    assert has("c05_ddpm_paired", variant=R.PAIRED_TAIL, grid=4) and has("c06_ddpm_tail_behind", variant=R.LAST_FINAL)
    assert has("c07_gen1_nw8", nw=8, block=512) and has("c07_gen1_nw4", nw=4, block=256)
    assert has("c07_family41", mode=R.POST, family=1) and has("c07_family41", mode=R.POST, variant=R.LAST_FINAL)
    assert has("c08_mt4_v4", family=4, mt=4, stream=R.S_TALL_WIDE) and has("c08_mt5_v4", family=4, mt=5, stream=R.S_TALL)
    assert has("c08_mt4_v1", family=1, mt=4, nw=8) and has("c08_mt5_v1", family=1, nw=4) and has("c08_mt2_v1", family=1, mt=2, nw=8)
    assert not has("c09_B13_T480", variant=R.MIX) and has("c09_B13_T480", mode=R.MID, mt=2, grid=390)
    assert has("c09_B26_T480_mix", mode=R.MID, variant=R.MIX, grid=512, n_tall=24) and not has("c09_B26_T480_mix", mode=R.PRE, variant=R.MIX)
    assert has("c09_B26_T480_mix_pre", mode=R.PRE, variant=R.MIX, grid=512, n_tall=24)
    assert has("c10_B26_T480_no_mix", mode=R.POST, variant=R.UNIFORM, mt=3, grid=520)
    assert has("c11_tail16", mode=R.POST, family=1) and has("c11_tail16", mode=R.MID, family=4) and not has("c11_tail16", mode=R.IN)
    assert has("c12_body_midpost", mode=R.MIDPOST, d=256, nw=8) and not has("c12_body_midpost", mode=R.POST)
    assert has("c13_body_no_fused_kf", mode=R.POST, d=256) and len(picks["c13_body_no_fused_kf"]) == 1 + 3 * R.MODELS["pose"]["L"]
    assert has("c14_body_nw4_mt6", mode=R.MIDPOST, mt=6, nw=4, block=256)


def test_every_case_takes_the_chain_path_and_fits_the_log():
    for c in R.CASES:
        assert R.takes_chain_path(c), c.name
        assert len(R.expected(c, family=(4, 4))["picks"]) <= R.MAX_PICKS, c.name
    assert len({c.name for c in R.CASES}) == len(R.CASES)
