"""SRTrainer's first steps, pinned: tests/golden/train_steps.json was recorded (tests/golden/make_train_steps_golden.py, twice,
byte-identical) BEFORE the trainer's capture / step code was folded into one path each, through names that exist on both sides of
that change.  The four cases - generators only and the G/D alternation, eager and replayed from hipGraphs - are run again here:
every loss and the final bits of every network, optimizer-updated buffer and EMA copy must equal the file, and the eager and the
replayed case of each pair must equal each other."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "train_steps.json")


@pytest.fixture(scope="module")
def steps():
    spec = importlib.util.spec_from_file_location("make_train_steps_golden", os.path.join(HERE, "golden", "make_train_steps_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(GOLDEN) as f:
        want = json.load(f)
    return mod.run_cases(), want


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["g_eager", "g_replay", "gd_eager", "gd_replay"])
def test_training_steps_equal_the_recorded_ones(steps, case):
    got, want = steps
    assert set(got) == set(want) == {"g_eager", "g_replay", "gd_eager", "gd_replay"}
    assert len(got[case]["losses"]) == len(want[case]["losses"]) == 6
    for k, (a, b) in enumerate(zip(got[case]["losses"], want[case]["losses"])):
        assert a == b, (case, "step %d" % k, a, b)
    assert got[case]["state"] == want[case]["state"], case


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["g", "gd"])
def test_eager_and_replayed_steps_are_the_same_bits(steps, pair):
    for which in steps:                                      # in this tree, and in the one the file was recorded from
        assert which[pair + "_eager"] == which[pair + "_replay"], pair
