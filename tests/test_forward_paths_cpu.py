"""The CPU half of the per-element forward tests (tests/test_forward_paths_hip.py): the instance list of the restatement against the source, the
coverage of the shallow cases, the gate's power against seeded faults and the committed envelope against a fresh run of the CPU model.
No GPU, no library.

Regenerate the envelope file after a change of oracle/lowprec_model.py or of the cases:  PYTHONPATH=. python tests/test_forward_paths_cpu.py --write"""
import json
import os
import re
import sys

import pytest

import chain_plan_restatement as R
import forward_paths_oracle as FP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"PRE": R.PRE, "MID": R.MID, "POST": R.POST, "MIDPOST": R.MIDPOST, "IN": R.IN}
VARIANTS = {"UNIFORM": R.UNIFORM, "MIX": R.MIX, "NEXT": R.NEXT, "LAST": R.LAST, "LAST_FINAL": R.LAST_FINAL, "PAIRED_TAIL": R.PAIRED_TAIL}


def test_instance_table_has_not_drifted():
    """INSTANCES is kChainInst, entry for entry: a new instance without a test fails here."""
    src = open(os.path.join(ROOT, "audio2photoreal_amd", "csrc", "a2p_lib_run.h")).read()
    table = src[src.index("static const ChainInst kChainInst[] = {"):]
    table = table[:table.index("#undef CI")]
    found = [(int(f), int(d), int(mt), int(nw), MODES[mode], VARIANTS[var])
             for f, d, mt, nw, mode, var in re.findall(r"\bCI\((\d+), (\d+), (\d+), (\d+), (\w+), (\w+)\)", table)]
    assert len(found) == len(set(found)) == table.count("CI("), "an entry the pattern does not read, or a duplicate"
    assert found == list(R.INSTANCES), set(found) ^ set(R.INSTANCES)


def test_every_instance_is_reached_by_a_shallow_case():
    reached = set()
    for case in R.SHALLOW_CASES:
        picks = [p[:6] for p in R.expected(case)["picks"]]
        assert picks == list(case.hits), (case.name, picks, case.hits)      # the rule and the launch pattern written beside the case agree
        reached.update(picks)
    assert len(R.NOT_REACHED) <= 4 and all(isinstance(v, str) and v for v in R.NOT_REACHED.values())
    assert not reached & set(R.NOT_REACHED), "an instance listed as unreachable is reached"
    assert reached | set(R.NOT_REACHED) == set(R.INSTANCES), set(R.INSTANCES) - reached - set(R.NOT_REACHED)
    assert len({c.name for c in R.SHALLOW_CASES}) == len(R.SHALLOW_CASES)


@pytest.mark.parametrize("name", ["face_S88_gen1_mt3_nw8", "pose_S88_midpost_mt3_nw8"])
def test_gate_sees_seeded_faults(name):
    """Oracle side only: the low-precision model's output passes the gate, and each seeded fault of it does not."""
    case, mode = R.SHALLOW_BY_NAME[name], "fp16"
    want = FP.reference(case)["out"]
    got = FP.lowprec_outputs(case, mode, "attn3")["out"]
    gate_max, gate_rms = (FP.MARGIN * v for v in FP.envelope(case, mode))
    mx, rm = FP.statistic(got, want)
    assert mx <= gate_max and rm <= gate_rms, (mx, rm, gate_max, gate_rms)
    faults = {"one row zeroed": FP.fault_zero_row(case, got),
              "FiLM of the previous sequence in a straddling panel": FP.fault_film_of_previous_sequence(case, mode, got),
              "stale rows in the ragged last panel": FP.fault_stale_last_panel(case, got),
              "16 columns of one row x (1 + 2^-6)": FP.fault_scaled_slice(case, got)}
    for what, bad in faults.items():
        mx, rm = FP.statistic(bad, want)
        assert mx > gate_max, (what, mx, gate_max)                          # (the local faults barely move the rms: the max is what sees them)


def _fresh_envelope(key, tail16):
    case = FP.envelope_cases()[(key, tail16)]
    return {FP.mode_of(p, tail16): FP.compute_envelope(case, FP.mode_of(p, tail16)) for p in ("fp16", "bf16")}


def _fresh_envelopes():
    out = {}
    for key, tail16 in FP.envelope_cases():
        out.setdefault(key, {}).update(_fresh_envelope(key, tail16))
    return out


def test_envelope_file_holds_the_shapes_of_the_cases_and_numbers_only():
    committed = FP.load_envelopes()
    want = {}
    for key, tail16 in FP.envelope_cases():
        want.setdefault(key, set()).update(FP.mode_of(p, tail16) for p in ("fp16", "bf16"))
    assert {k: set(v) for k, v in committed.items()} == want
    for modes in committed.values():
        for outs in modes.values():
            assert all(len(v) == 2 and all(isinstance(x, float) and 0.0 < x < 0.1 for x in v) for v in outs.values()), outs


@pytest.mark.parametrize("key,tail16", sorted(FP.envelope_cases()))
def test_envelope_file_is_reproducible(key, tail16):
    """tests/golden/forward_paths_envelope.json holds the low-precision model's own statistic per (case shape, mode); the GPU test reads it instead of
    running the model.  A fresh run of the model agrees within 1 %."""
    committed = FP.load_envelopes()[key]
    for mode, outs in _fresh_envelope(key, tail16).items():
        assert set(outs) == set(committed[mode]), (key, mode)
        for name, vals in outs.items():
            for got, want in zip(vals, committed[mode][name]):
                assert abs(got - want) <= 0.01 * want, (key, mode, name, vals, committed[mode][name])


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        env = _fresh_envelopes()
        env = {k: {m: {n: [float(f"{x:.6e}") for x in v] for n, v in o.items()} for m, o in ms.items()} for k, ms in env.items()}
        with open(FP.ENVELOPE_FILE, "w") as f:
            json.dump(env, f, indent=1, sort_keys=True)
        print(json.dumps(env, indent=1, sort_keys=True))
