#!/usr/bin/env python3
"""Recovers the orientation of a captured environment, and then the environment itself, on dirt_amd (MI355X): the glossy sphere
of fit_material_environment_fused.py in front of its environment, as fit_environment_background_fused.py renders it, but lit by
a lat-long (equirectangular) PANORAMA, the form environments are captured in.  `texture.panorama_to_cube` stands at the head of
the chain and turns the panorama into the cube every other stage takes, under a rotation:

    panorama, angle -> panorama_to_cube(rotation=rodrigues(angle)) -> prefilter_cube / convolve_cube
        -> shade_gbuffer_ibl + environment_background -> loss

Two descents:

  1. on the angle-axis vector of the rotation, three numbers, from a wrong start, with the panorama known;
  2. on the panorama itself, with the rotation fixed at the truth: the gradient arrives through the same head.

The recovered environment is written back as a panorama by `texture.cube_to_panorama`.

    python examples/fit_environment_rotation_fused.py
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from dirt_amd import lighting, matrices, texture  # noqa: E402
from fit_environment_background_fused import render  # noqa: E402
from fit_environment_fused import SIZE  # noqa: E402
from fit_material_environment_fused import TABLE, Scene  # noqa: E402

PANORAMA = (32, 64)                   # rows, columns of the panorama
SAMPLES = 2                           # look-ups per cube texel, each way
TRUE_ANGLE = (0.15, 0.5, -0.1)        # the environment's rotation the first descent looks for (angle-axis, radians)


def true_panorama(device):
    """A sky in lat-long form: blue above, brown below, a warm sun up to one side and a cooler lamp low on another"""
    d, _ = texture.panorama_texel_directions(*PANORAMA)
    up = d[..., 1:2]
    sky = torch.tensor([0.3, 0.5, 0.9]) * (0.5 + 0.5 * up) + torch.tensor([0.35, 0.25, 0.15]) * (0.5 - 0.5 * up)
    unit = lambda v: torch.nn.functional.normalize(torch.tensor(v), dim=0)   # noqa: E731
    sun = torch.exp(6. * (d @ unit([1., 1., -0.5]) - 1.))[..., None] * torch.tensor([1.0, 0.8, 0.5])
    lamp = torch.exp(4. * (d @ unit([-1., -0.2, -0.6]) - 1.))[..., None] * torch.tensor([0.2, 0.7, 0.6])
    return (sky + sun + lamp).to(device)


def environment(panorama, angle):
    """the cube the chain takes, from the panorama turned by the angle-axis `angle` [3]"""
    return texture.panorama_to_cube(panorama, SIZE, samples=SAMPLES, rotation=matrices.rodrigues(angle, three_by_three=True))


def angle_between(a, b):
    """the angle of the rotation that takes rodrigues(a) to rodrigues(b), in radians"""
    r = matrices.rodrigues(a, three_by_three=True) @ matrices.rodrigues(b, three_by_three=True).transpose(-1, -2)
    return float(torch.acos(((r.diagonal().sum() - 1.) / 2.).clamp(-1., 1.)))


def fit_rotation(width=160, height=120, steps=60, rate=0.03, device=None):
    """-> (losses per step, the angle to the true rotation before and after)"""
    dev = device or torch.device('cuda', 0)
    scene, brdf, panorama = Scene(dev), lighting.environment_brdf(TABLE).to(dev), true_panorama(dev)
    truth = torch.tensor(TRUE_ANGLE, device=dev)
    target = render(scene, environment(panorama, truth), brdf, width, height).detach()
    angle = torch.zeros(3, device=dev, requires_grad=True)
    optimiser = torch.optim.Adam([angle], lr=rate)
    before = angle_between(angle.detach(), truth)
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        loss = ((render(scene, environment(panorama, angle), brdf, width, height) - target) ** 2).mean()
        loss.backward()
        optimiser.step()
        losses.append(float(loss.detach()))
    return losses, before, angle_between(angle.detach(), truth)


def fit_panorama(width=160, height=120, steps=60, rate=0.05, device=None):
    """-> (losses per step, mean |panorama - truth| before and after, the recovered environment written back as a panorama)"""
    dev = device or torch.device('cuda', 0)
    scene, brdf, truth = Scene(dev), lighting.environment_brdf(TABLE).to(dev), true_panorama(dev)
    angle = torch.tensor(TRUE_ANGLE, device=dev)
    target = render(scene, environment(truth, angle), brdf, width, height).detach()
    panorama = torch.full_like(truth, 0.5).requires_grad_(True)
    optimiser = torch.optim.Adam([panorama], lr=rate)
    before = float((panorama.detach() - truth).abs().mean())
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        loss = ((render(scene, environment(panorama, angle), brdf, width, height) - target) ** 2).mean()
        loss.backward()
        optimiser.step()
        with torch.no_grad():
            panorama.clamp_(min=0.)
        losses.append(float(loss.detach()))
    with torch.no_grad():      # the environment as the renderer saw it, back in the form it was captured in
        rotation = matrices.rodrigues(angle, three_by_three=True)
        written = texture.cube_to_panorama(environment(panorama, angle), *PANORAMA, samples=SAMPLES, rotation=rotation)
    return losses, before, float((panorama.detach() - truth).abs().mean()), written


def main():
    losses, before, after = fit_rotation()
    print('rotation: losses ' + ' '.join('%.3e' % x for x in losses[::10] + losses[-1:]))
    print('loss %.3e -> %.3e in %d steps; angle to the true rotation %.1f -> %.1f degrees' % (
        losses[0], losses[-1], len(losses), math.degrees(before), math.degrees(after)))
    assert losses[-1] < losses[0] and after < before, 'the fit did not bring the loss and the angle down'
    losses, before, after, written = fit_panorama()
    print('panorama: losses ' + ' '.join('%.3e' % x for x in losses[::10] + losses[-1:]))
    print('loss %.3e -> %.3e in %d steps; mean |panorama - truth| %.3f -> %.3f; written back as %s' % (
        losses[0], losses[-1], len(losses), before, after, tuple(written.shape)))
    assert losses[-1] < losses[0] and after < before, 'the fit did not bring the loss and the panorama error down'


if __name__ == '__main__':
    main()
