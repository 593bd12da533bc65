"""examples/fit_environment_background_fused.py at a reduced size: each of its two descents brings its loss below the share of
its start that the example itself asserts."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    spec = importlib.util.spec_from_file_location('examples_fit_environment_background_fused',
                                                  os.path.join(ROOT, 'examples', 'fit_environment_background_fused.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_the_environment_behind_the_sphere_is_recovered(gpu):
    ex = _example()
    losses, before, after = ex.fit_environment(width=64, height=48, steps=30, device=gpu)
    print('%.3e -> %.3e, behind %.3f -> %.3f' % (losses[0], losses[-1], before, after))
    assert losses[-1] < ex.ENVIRONMENT_FRACTION * losses[0] and after < before


@pytest.mark.gpu
def test_the_camera_turns_towards_the_truth_from_the_background_alone(gpu):
    ex = _example()
    losses, before, after = ex.fit_camera(width=64, height=48, steps=40, device=gpu)
    print('%.3e -> %.3e, angle %.3f -> %.3f' % (losses[0], losses[-1], before, after))
    assert losses[-1] < ex.CAMERA_FRACTION * losses[0] and after < before
