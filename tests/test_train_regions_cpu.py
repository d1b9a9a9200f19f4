"""scda_amd.train_step.run_region: the one place that runs a GAN region eagerly, records it or replays it, copies the outputs that
outlive the next replay and decides who issues the region's all-reduces -- driven with stand-ins: no trainer, no device."""
import pytest
import torch

from scda_amd.train_step import REGIONS, run_region


class StubGraphs:
    """what run_region needs of _GanGraphs: ready / recording / record / run; `static` stands for the recorded input tensors"""

    def __init__(self, log, ready=(), recording=True, n_out=4):
        self.log, self._ready, self._recording = log, set(ready), recording
        self.static = {"x": torch.full((3,), 7.0)}
        self.out = tuple(torch.arange(4.0) + i for i in range(n_out))

    def ready(self, name):
        return name in self._ready

    def recording(self):
        return self._recording

    def record(self, name, t, fn):
        self.log.append(("record", name))
        out = fn(self.static)
        self.log.append(("replay", name))
        return out

    def run(self, name, t):
        self.log.append(("replay", name))
        return self.out


N_OUT = {'a': 4, 'b': 3, 'c': 2}


def _harness(n_out, fail=False):
    log = []

    def all_reduce(net):
        log.append(("all_reduce", net))
        return "work:" + net

    def fn(t, reduce):
        log.append(("fn", t))
        if fail:
            raise ValueError("inside the region")
        reduce('dis')
        log.append(("between",))
        reduce('dis_patch')
        fn.out = tuple(torch.arange(4.0) * (i + 2) for i in range(n_out))
        return fn.out
    return log, all_reduce, fn


def test_the_table_of_regions():
    assert REGIONS == {
        'a': {'keys': ('src_patch', 'tgt_patch', 'x_small', 't_small', 'score1', 'score0', 'score0p', 'score1p'),
              'copies': (2, 3), 'nets': ('dis', 'dis_patch')},
        'b': {'keys': ('x_small', 't_small', 'tgt_patch', 'one_t', 'zero_t', 'one_s', 'zero_s'), 'copies': (0, 1), 'nets': ('dec',)},
        'c': {'keys': ('src_patch', 'tgt_patch', 'ones_all', 'ones_row'), 'copies': (0, 1), 'nets': ()}}


@pytest.mark.parametrize("graphs", [None, "warming up"])
def test_eager_fn_gets_t_and_issues_its_own_all_reduces(graphs):
    log, all_reduce, fn = _harness(4)
    if graphs is not None:          # a graphs object in its two eager iterations changes nothing
        graphs = StubGraphs(log, recording=False)
    t = {"x": torch.zeros(3)}
    out, works = run_region(graphs, 'a', t, fn, all_reduce)
    assert log[0][0] == "fn" and log[0][1] is t
    assert log[1:] == [("all_reduce", "dis"), ("between",), ("all_reduce", "dis_patch")]       # ... where fn asked for them
    assert out is fn.out and works == {"dis": "work:dis", "dis_patch": "work:dis_patch"}


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_a_ready_region_is_replayed_copied_by_the_table_and_reduced_behind_the_replay(name):
    log, all_reduce, fn = _harness(N_OUT[name])
    g = StubGraphs(log, ready=(name,), n_out=N_OUT[name])
    out, works = run_region(g, name, {"x": torch.zeros(3)}, fn, all_reduce)
    nets = REGIONS[name]['nets']
    assert log == [("replay", name)] + [("all_reduce", n) for n in nets]             # fn not called; once per net, in table order
    assert works == {n: "work:" + n for n in nets}
    assert len(out) == N_OUT[name]
    for i, (o, rec) in enumerate(zip(out, g.out)):
        if i in REGIONS[name]['copies']:
            assert torch.equal(o, rec) and o.data_ptr() != rec.data_ptr()
        else:
            assert o is rec


def test_a_recording_region_gets_the_recorded_inputs_and_issues_nothing_itself():
    log, all_reduce, fn = _harness(4)
    g = StubGraphs(log)
    out, works = run_region(g, 'a', {"x": torch.zeros(3)}, fn, all_reduce)
    assert log[0] == ("record", "a") and log[1][0] == "fn" and log[1][1] is g.static
    assert log[2:] == [("between",), ("replay", "a"), ("all_reduce", "dis"), ("all_reduce", "dis_patch")]
    assert works == {"dis": "work:dis", "dis_patch": "work:dis_patch"}
    assert out[0] is fn.out[0] and out[1] is fn.out[1]
    assert all(torch.equal(out[i], fn.out[i]) and out[i].data_ptr() != fn.out[i].data_ptr() for i in (2, 3))


@pytest.mark.parametrize("recording", [False, True])
def test_a_region_that_raises_leaves_nothing_behind(recording):
    """an exception inside a region (an out-of-memory error while recording, a shape error) propagates, and the eager call after it
    issues its all-reduces inside fn as ever: there is no flag an exception could leave set"""
    log, all_reduce, bad = _harness(4, fail=True)
    with pytest.raises(ValueError, match="inside the region"):
        run_region(StubGraphs(log) if recording else None, 'a', {}, bad, all_reduce)
    assert not any(e[0] == "all_reduce" for e in log)
    log, all_reduce, fn = _harness(4)
    out, works = run_region(None, 'a', {}, fn, all_reduce)
    assert [e[0] for e in log] == ["fn", "all_reduce", "between", "all_reduce"] and sorted(works) == ["dis", "dis_patch"]
