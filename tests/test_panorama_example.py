"""examples/fit_environment_rotation_fused.py at a small size: a 64 x 48 image, a few tens of steps."""
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
def test_the_rotation_of_the_environment_is_found(gpu):
    """The final loss is below the initial one, and the final angle to the true rotation below the initial one"""
    ex = _load('examples', 'fit_environment_rotation_fused')
    losses, before, after = ex.fit_rotation(width=64, height=48, steps=40, rate=0.03, device=gpu)
    print('loss %.3e -> %.3e, angle to the true rotation %.3f -> %.3f rad' % (losses[0], losses[-1], before, after))
    assert losses[-1] < losses[0] and after < before


@pytest.mark.gpu
def test_the_panorama_descends_and_is_written_back(gpu):
    """The gradient reaches the panorama through the head of the chain: the loss and the panorama's error fall; the recovered
    environment comes back in the panorama's own shape"""
    ex = _load('examples', 'fit_environment_rotation_fused')
    losses, before, after, written = ex.fit_panorama(width=64, height=48, steps=30, rate=0.05, device=gpu)
    print('loss %.3e -> %.3e, mean |panorama - truth| %.3f -> %.3f' % (losses[0], losses[-1], before, after))
    assert losses[-1] < losses[0] and after < before
    assert tuple(written.shape) == ex.PANORAMA + (3,) and bool(written.isfinite().all())
