#!/usr/bin/env python3
"""The glossy sphere of fit_material_environment_fused.py in front of its environment, on dirt_amd (MI355X): where the mesh does
not cover a pixel the image shows the environment itself, by `shading.environment_background`, in place of a flat backdrop.
One `rasterise_deferred` call whose shader is

    shade_gbuffer_ibl(gbuffer, pyramid, irradiance, brdf, ..., background=(0, 0, 0), clamp=None)
        + environment_background(pyramid, clip_to_world, (height, width), mask=gbuffer[..., 0], filter='trilinear')

with the ONE pyramid of `texture.prefilter_cube`: its level 0 is the environment, which the background reads at the level of
detail of each pixel's own footprint, while the sphere reads the rougher levels.  Two short descents:

  1. on the environment cube, from an image of the sphere in front of it: the texels behind the sphere, which no reflection
     shows sharply, are read off the background directly;
  2. on a small rotation of the camera, from the background alone: each pixel looks at a few texels, so the image moves with
     the camera by its whole gradient.

    python examples/fit_environment_background_fused.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import lighting, matrices, shading, texture  # noqa: E402
from fit_environment_fused import CAMERA, SIZE, true_environment  # noqa: E402
from fit_material_environment_fused import CHANNELS, LAYOUT, TABLE, Scene, filtered  # noqa: E402

TRUE_ANGLE = (0.05, -0.08, 0.03)      # the camera's rotation the second descent looks for (angle-axis, radians)
ENVIRONMENT_FRACTION = 0.5            # what each descent's loss must fall below, as a share of its start
CAMERA_FRACTION = 0.1


def clip_to_world(angle, width, height):
    """inverse(view @ projection) of the camera at CAMERA turned by the angle-axis `angle` [3]: the projection is a constant,
    inverted once on the host; the view's inverse is written out, so the matrix is differentiable in the angle"""
    projection = matrices.perspective_projection(near=0.1, far=20., right=0.05, aspect=float(height) / width)
    unproject = torch.linalg.inv(projection.double()).float().to(angle.device)
    return unproject @ matrices.rodrigues(angle).transpose(-1, -2) @ matrices.translation(torch.tensor(CAMERA, device=angle.device))


def render(scene, environment, brdf, width, height, keep=None):
    """The sphere lit by the environment, in front of it.  keep: a list the shader's G-buffer is appended to"""
    inverse = clip_to_world(torch.zeros(3, device=environment.device), width, height)

    def shader_fn(gbuffer, env):
        if keep is not None:
            keep.append(gbuffer)
        pyramid, irradiance = filtered(env)
        lit = shading.shade_gbuffer_ibl(gbuffer, pyramid, irradiance, brdf, camera_position=CAMERA, background=(0., 0., 0.), clamp=None, **LAYOUT)
        behind = shading.environment_background(pyramid, inverse, (height, width), mask=gbuffer[..., LAYOUT['mask']], filter='trilinear')
        return (lit + behind).clamp(0., 1.)

    return dirt.rasterise_deferred(background_attributes=torch.zeros([height, width, CHANNELS], device=environment.device),
                                   vertices=scene.clip(width, height), vertex_attributes=scene.attributes(), faces=scene.faces,
                                   shader_fn=shader_fn, shader_additional_inputs=[environment])


def fit_environment(width=160, height=120, steps=60, rate=0.05, device=None):
    """-> (losses per step, mean |environment - truth| over the texels the background looks at, before and after)"""
    dev = device or torch.device('cuda', 0)
    scene = Scene(dev)
    brdf = lighting.environment_brdf(TABLE).to(dev)
    truth = true_environment(SIZE, dev)
    gbuffers = []
    target = render(scene, truth, brdf, width, height, keep=gbuffers).detach()
    # the texels behind the sphere: those the background's look-ups touch
    probe = truth.clone().requires_grad_(True)
    inverse = clip_to_world(torch.zeros(3, device=dev), width, height)
    shading.environment_background(probe, inverse, (height, width), mask=gbuffers[0][..., LAYOUT['mask']].detach()).sum().backward()
    behind = probe.grad != 0
    environment = torch.full_like(truth, 0.5).requires_grad_(True)
    optimiser = torch.optim.Adam([environment], lr=rate)
    before = float((environment.detach() - truth).abs()[behind].mean())
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        loss = ((render(scene, environment, brdf, width, height) - target) ** 2).mean()
        loss.backward()
        optimiser.step()
        with torch.no_grad():
            environment.clamp_(min=0.)
        losses.append(float(loss.detach()))
    return losses, before, float((environment.detach() - truth).abs()[behind].mean())


def fit_camera(width=160, height=120, steps=40, rate=0.01, device=None):
    """-> (losses per step, |angle - truth| before and after): the rotation of the camera from the background alone"""
    dev = device or torch.device('cuda', 0)
    pyramid = texture.prefilter_cube(true_environment(SIZE, dev))
    truth = torch.tensor(TRUE_ANGLE, device=dev)
    target = shading.environment_background(pyramid, clip_to_world(truth, width, height), (height, width), filter='trilinear').detach()
    angle = torch.zeros(3, device=dev, requires_grad=True)
    optimiser = torch.optim.Adam([angle], lr=rate)
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        image = shading.environment_background(pyramid, clip_to_world(angle, width, height), (height, width), filter='trilinear')
        loss = ((image - target) ** 2).mean()
        loss.backward()
        optimiser.step()
        losses.append(float(loss.detach()))
    return losses, float(truth.norm()), float((angle.detach() - truth).norm())


def main():
    losses, before, after = fit_environment()
    print('environment: losses ' + ' '.join('%.3e' % x for x in losses[::10] + losses[-1:]))
    print('loss %.3e -> %.3e in %d steps; mean |environment - truth| behind the sphere %.3f -> %.3f' % (losses[0], losses[-1], len(losses), before, after))
    assert losses[-1] < ENVIRONMENT_FRACTION * losses[0] and after < before, 'the fit did not bring the loss and the texels behind the sphere down'
    losses, before, after = fit_camera()
    print('camera: losses ' + ' '.join('%.3e' % x for x in losses[::10] + losses[-1:]))
    print('loss %.3e -> %.3e in %d steps; |angle - truth| %.3f -> %.3f' % (losses[0], losses[-1], len(losses), before, after))
    assert losses[-1] < CAMERA_FRACTION * losses[0], 'the fit did not bring the loss down'


if __name__ == '__main__':
    main()
