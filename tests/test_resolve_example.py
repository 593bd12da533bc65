"""examples/fit_exposure_fused.py at a small size: a 64 x 64 render resolved to 32 x 32, a few tens of steps."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(folder, name):
    spec = importlib.util.spec_from_file_location('%s_%s' % (folder, name), os.path.join(ROOT, folder, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_the_gains_are_found_from_an_srgb_target(gpu):
    """The three gains end closer to the target's than they started, and the loss lower"""
    ex = _load('examples', 'fit_exposure_fused')
    losses, before, after = ex.fit_gains(width=32, height=32, steps=30, rate=0.05, device=gpu)
    print('loss %.3e -> %.3e, |gains - truth| %.3f -> %.3f' % (losses[0], losses[-1], before, after))
    assert after < before and losses[-1] < losses[0]


@pytest.mark.gpu
def test_the_environment_descends_through_the_whole_chain(gpu):
    """The gradient reaches the environment through the encode, the curve, the gains and the resolve: the loss falls"""
    ex = _load('examples', 'fit_exposure_fused')
    losses = ex.fit_environment(width=32, height=32, steps=20, rate=0.05, device=gpu)
    print('loss %.3e -> %.3e' % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
