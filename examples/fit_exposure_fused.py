#!/usr/bin/env python3
"""The glossy sphere of fit_environment_background_fused.py in front of its environment, developed like a photograph, on
dirt_amd (MI355X): rendered at twice the size as linear HDR radiance and brought to an sRGB image by one call,

    resolve_image(shade_gbuffer_ibl(..., background=(0, 0, 0), clamp=None), add=environment_background(..., mask=gbuffer[..., 0]),
                  factor=2, exposure=gains, curve='aces', encode='srgb')

which adds the two radiance images, box-filters 2 x 2 samples into a pixel, applies the three gains (exposure and white
balance), the ACES curve, the sRGB transfer function and the clamp.  Two short descents against an sRGB target made with other
gains:

  1. on the three gains, the environment known;
  2. on the environment cube through the whole chain, the gains known: the over-exposed pixels, which a hard clamp of the
     radiance would cut off from the loss, pass their gradient through the curve.

    python examples/fit_exposure_fused.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import lighting, shading  # noqa: E402
from fit_environment_background_fused import clip_to_world  # noqa: E402
from fit_environment_fused import CAMERA, SIZE, true_environment  # noqa: E402
from fit_material_environment_fused import CHANNELS, LAYOUT, TABLE, Scene, filtered  # noqa: E402

FACTOR = 2                          # samples per pixel, each way
TRUE_GAINS = (1.6, 1.1, 0.7)        # the target's exposure per channel
GAINS_FRACTION = 0.1                # what each descent's loss must fall below, as a share of its start
ENVIRONMENT_FRACTION = 0.5


def develop(scene, environment, brdf, gains, width, height):
    """The sphere lit by the environment, in front of it: rendered at FACTOR times (height, width), -> sRGB [height, width, 3]"""
    W, H = FACTOR * width, FACTOR * height
    dev = environment.device
    gbuffer = dirt.rasterise(torch.zeros([H, W, CHANNELS], device=dev), scene.clip(W, H), scene.attributes(), scene.faces)
    pyramid, irradiance = filtered(environment)
    lit = shading.shade_gbuffer_ibl(gbuffer, pyramid, irradiance, brdf, camera_position=CAMERA, background=(0., 0., 0.), clamp=None, **LAYOUT)
    behind = shading.environment_background(pyramid, clip_to_world(torch.zeros(3, device=dev), W, H), (H, W), mask=gbuffer[..., LAYOUT['mask']],
                                            filter='trilinear')
    return shading.resolve_image(lit, add=behind, factor=FACTOR, exposure=gains, curve='aces', encode='srgb')


def descend(parameter, image_of, target, steps, rate, floor=None):
    optimiser = torch.optim.Adam([parameter], lr=rate)
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        loss = ((image_of() - target) ** 2).mean()
        loss.backward()
        optimiser.step()
        if floor is not None:
            with torch.no_grad():
                parameter.clamp_(min=floor)
        losses.append(float(loss.detach()))
    return losses


def fit_gains(width=160, height=120, steps=60, rate=0.05, device=None):
    """-> (losses per step, |gains - truth| before and after)"""
    dev = device or torch.device('cuda', 0)
    scene, brdf, environment = Scene(dev), lighting.environment_brdf(TABLE).to(dev), true_environment(SIZE, dev)
    truth = torch.tensor(TRUE_GAINS, device=dev)
    target = develop(scene, environment, brdf, truth, width, height).detach()
    gains = torch.ones(3, device=dev, requires_grad=True)
    before = float((gains.detach() - truth).norm())
    losses = descend(gains, lambda: develop(scene, environment, brdf, gains, width, height), target, steps, rate, floor=0.01)
    return losses, before, float((gains.detach() - truth).norm())


def fit_environment(width=160, height=120, steps=60, rate=0.05, device=None):
    """-> losses per step: the environment through the resolve, the curve and the encoding, the gains known"""
    dev = device or torch.device('cuda', 0)
    scene, brdf = Scene(dev), lighting.environment_brdf(TABLE).to(dev)
    truth = torch.tensor(TRUE_GAINS, device=dev)
    target = develop(scene, true_environment(SIZE, dev), brdf, truth, width, height).detach()
    environment = torch.full((6, SIZE, SIZE, 3), 0.5, device=dev).requires_grad_(True)
    return descend(environment, lambda: develop(scene, environment, brdf, truth, width, height), target, steps, rate, floor=0.)


def main():
    losses, before, after = fit_gains()
    print('gains: losses ' + ' '.join('%.3e' % x for x in losses[::10] + losses[-1:]))
    print('loss %.3e -> %.3e in %d steps; |gains - truth| %.3f -> %.3f' % (losses[0], losses[-1], len(losses), before, after))
    assert losses[-1] < GAINS_FRACTION * losses[0] and after < before, 'the fit did not bring the loss and the gains down'
    losses = fit_environment()
    print('environment: losses ' + ' '.join('%.3e' % x for x in losses[::10] + losses[-1:]))
    assert losses[-1] < ENVIRONMENT_FRACTION * losses[0], 'the fit did not bring the loss down'


if __name__ == '__main__':
    main()
