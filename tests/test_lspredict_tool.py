"""tools/ls_predict_replay.py: the replay of the line search's predictor
(ls_phase, BSGP_LS_PREDICT) on outcome strings.  CPU only."""
import importlib.util
import os

from conftest import ROOT


def test_replay_tool_predictor_on_recorded_outcomes():
    """Outcome strings recorded from the oracle (bench-generator seeds 10000
    and 10005, MAXIT 100)."""
    spec = importlib.util.spec_from_file_location(
        "ls_predict_replay", os.path.join(ROOT, "tools", "ls_predict_replay.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    assert t.outcomes([1, 1, 2, 5, 11, 12, 23, 1]) == "AAMMMSSA"
    assert t.step_of(3) == 0.4 * 0.4 and t.step_of(1) == 1.0
    assert [t.predict(t.step_of(n)) for n in (1, 2, 11, 12, 30)] == ["A", "-", "-", "S", "S"]
    s0 = "A" * 12 + "M" + "A" * 16 + "MMMMM" + "S" * 66
    r = t.score(s0)
    assert (r["n"], r["pred_A"], r["hit_A"], r["pred_S"], r["hit_S"], r["none"]) == \
        (100, 29, 27, 65, 65, 6)
    assert r["hit_rate"] == 0.92
    s5 = "A" * 24 + "M" + "A" * 5 + "MSMM" + "S" * 66
    r = t.score(s5)
    assert (r["pred_A"], r["hit_A"], r["pred_S"], r["hit_S"], r["none"]) == (30, 28, 66, 65, 4)
