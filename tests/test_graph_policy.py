"""train.GraphPolicy (TGSR_GRAPH_G=auto) driven through a whole run with an injected clock: no device.

Expected sequences, from the schedule the trainer has always had (GRAPH_G_WARMUP = 3, GRAPH_G_TRIALS = 3, GRAPH_G_SETTLED = 10):
steps 0-2 warm up (eager, untimed), 3-5 are timed eager, step 6 has the replayed form but captures and is not timed, 7-9 are timed
replays; the end of step 9 decides by the medians, `replay` iff its median <= the eager one; a replay trial that did not really
replay counts as inf; with no eager time the first guess stands; an explicit choice ends the measurement and reports nothing chosen.
"""
import pytest

from tgsr_amd import train

INF = float("inf")
EAGER_STEPS = train.GRAPH_G_WARMUP + train.GRAPH_G_TRIALS                     # 6
TIMED = [3, 4, 5, 7, 8, 9]

# name, prior, seconds an eager / a replayed step takes, replay trials really replayed, eager trials that get their clock read,
# pinned at step (-> value), expected chosen form, expected (eager_ms, replay_ms)
CASES = [
    ("replay faster", False, 0.012, 0.010, True, True, None, "replay", (12.0, 10.0)),
    ("eager faster", True, 0.010, 0.012, True, True, None, "eager", (10.0, 12.0)),
    ("tie chooses replay", False, 0.015625, 0.015625, True, True, None, "replay", (15.625, 15.625)),   # (2^-6 s: sums stay exact)
    ("failed capture", True, 0.012, 0.010, False, True, None, "eager", (12.0, None)),
    ("no eager time: the first guess stands", True, 0.012, 0.010, True, False, None, "replay", None),
    ("pinned at step 4", False, 0.012, 0.010, True, True, (4, True), None, None),
]


@pytest.mark.parametrize("name,prior,t_eager,t_replay,replayed,eager_ends,pin,chosen,ms", CASES, ids=[c[0] for c in CASES])
def test_measured_graph_policy_schedule_and_decision(name, prior, t_eager, t_replay, replayed, eager_ends, pin, chosen, ms):
    assert (train.GRAPH_G_WARMUP, train.GRAPH_G_TRIALS, train.GRAPH_G_SETTLED) == (3, 3, 10)
    now = [0.0]
    reads = []                                     # the step during which each clock reading was taken

    def clock():
        reads.append(step)
        return now[0]

    pol = train.GraphPolicy("auto", prior=prior, measuring=True, clock=clock)
    assert pol.report == {"mode": "auto", "prior": "replay" if prior else "eager"} and pol.graph == prior
    forms, took = [], []
    for step in range(train.GRAPH_G_SETTLED + 1):
        if pin is not None and step == pin[0]:
            pol.pin(pin[1])
        pol.begin(step)
        forms.append(pol.form if pol.measuring else None)
        replays = pol.replays(step)
        took.append(replays)
        now[0] += t_replay if replays else t_eager
        if replays or eager_ends:                  # (an eager step that raised never reaches its end)
            pol.end(step, replays and replayed)
    settled = train.GRAPH_G_SETTLED if pin is None else pin[0]
    assert forms[:settled] == (["eager"] * EAGER_STEPS + ["replay"] * (train.GRAPH_G_SETTLED - EAGER_STEPS))[:settled], forms
    assert forms[settled:] == [None] * (len(forms) - settled), forms
    assert not pol.measuring
    # the timed steps: a reading at the top and one at the end, none in any other step
    timed = [k for k in TIMED if k < settled]
    ends = [k for k in timed if k >= EAGER_STEPS or eager_ends]
    assert reads == sorted(timed + ends), reads
    # warm-up and eager trials run eager, the capturing step and the replay trials take the graphs, then the chosen form
    final = pin[1] if pin is not None else chosen == "replay"
    assert took[:settled] == ([False] * EAGER_STEPS + [True] * 4)[:settled], took
    assert took[settled:] == [final and k >= train.GRAPH_G_WARMUP for k in range(settled, len(took))], took
    assert pol.graph == final
    if pin is not None:
        assert pol.report == {"mode": "auto", "prior": "eager"}                 # nothing measured to the end, nothing chosen
        return
    assert pol.report["chosen"] == chosen
    if ms is None:
        assert set(pol.report) == {"mode", "prior", "chosen"} and chosen == ("replay" if prior else "eager")
        return
    assert set(pol.report) == {"mode", "prior", "chosen", "eager_ms", "replay_ms", "trials"}
    assert pol.report["eager_ms"] == pytest.approx(ms[0], abs=1e-3)
    assert pol.report["replay_ms"] is None if ms[1] is None else pol.report["replay_ms"] == pytest.approx(ms[1], abs=1e-3)
    assert pol.report["trials"] == "median of 3 steps of each form, device idle on both sides"
    assert pol.eager_s == pytest.approx([t_eager] * 3) and pol.replay_s == ([INF] * 3 if not replayed else pytest.approx([t_replay] * 3))


def test_unmeasured_policy_keeps_its_form():
    """TGSR_GRAPH_G=0 / 1: nothing is measured, no clock is read, the form only waits for the warm-up."""
    def clock():
        raise AssertionError("an unmeasured policy reads no clock")
    for graph in (False, True):
        pol = train.GraphPolicy("1" if graph else "0", prior=graph, measuring=False, clock=clock)
        for step in range(train.GRAPH_G_SETTLED + 1):
            pol.begin(step)
            assert pol.replays(step) == (graph and step >= train.GRAPH_G_WARMUP)
            pol.end(step, graph)
        assert pol.report == {"mode": "1" if graph else "0", "prior": "replay" if graph else "eager"}
