"""ops._check_wgrad, the one place that answers a weight gradient's SYNTHSR_EWORKSPACE (-3): host logic, no GPU (the launches
themselves: tests/test_wgrad_scratch_gpu.py)."""
import pytest

from synthsr_amd import _lib, ops


class _Fake:
    """a weight-gradient launch that returns the given codes in turn, and a stand-in for ops._register_det_planes"""

    def __init__(self, monkeypatch, codes, deterministic, short=True):
        self.codes, self.calls, self.registered = list(codes), 0, []
        monkeypatch.setattr(ops, '_deterministic', deterministic)
        monkeypatch.setattr(ops, '_register_det_planes', lambda n: (self.registered.append(n), short)[1])

    def __call__(self):
        self.calls += 1
        return self.codes.pop(0)


def test_eworkspace_in_deterministic_mode_registers_once_and_repeats_once(monkeypatch):
    f = _Fake(monkeypatch, [-3, 0], True)
    ops._check_wgrad(f, 'wgrad')
    assert f.calls == 2 and f.registered == [0]


def test_a_second_eworkspace_names_the_plane_buffer(monkeypatch):
    f = _Fake(monkeypatch, [-3, -3, 0], True)
    with pytest.raises(_lib.SynthSRHipError) as e:
        ops._check_wgrad(f, 'wgrad')
    assert f.calls == 2 and f.registered == [0]
    assert 'plane buffer' in str(e.value) and 'synthsr_set_deterministic_workspace' in str(e.value)
    assert 'conv context' not in str(e.value)


def test_eworkspace_with_sufficient_planes_is_about_the_conv_context(monkeypatch):
    """the registration already covered the demand: the -3 came from the context's workspace (the c2 kernel's partials)"""
    f = _Fake(monkeypatch, [-3, -3], True, short=False)
    with pytest.raises(_lib.SynthSRHipError, match='conv context') as e:
        ops._check_wgrad(f, 'wgrad')
    assert 'plane buffer' not in str(e.value)


def test_eworkspace_outside_deterministic_mode_raises_without_a_repeat(monkeypatch):
    f = _Fake(monkeypatch, [-3, 0], False)
    with pytest.raises(_lib.SynthSRHipError, match='conv context'):
        ops._check_wgrad(f, 'wgrad')
    assert f.calls == 1 and f.registered == []


@pytest.mark.parametrize('deterministic', [True, False])
def test_success_never_registers(monkeypatch, deterministic):
    f = _Fake(monkeypatch, [0], deterministic)
    ops._check_wgrad(f, 'wgrad')
    assert f.calls == 1 and f.registered == []


def test_other_errors_pass_through(monkeypatch):
    f = _Fake(monkeypatch, [-1], True)
    with pytest.raises(ValueError):
        ops._check_wgrad(f, 'wgrad')
    assert f.calls == 1 and f.registered == []


def test_the_two_eworkspace_causes_have_distinct_texts():
    texts = []
    for planes in (False, True):
        with pytest.raises(_lib.SynthSRHipError) as e:
            _lib.check(-3, 'wgrad', planes=planes)
        texts.append(str(e.value))
    assert texts[0] != texts[1] and 'synthsr_conv_ctx.workspace' in texts[0] and 'synthsr_hip_tuning.h' in texts[1]
