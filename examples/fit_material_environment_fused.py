#!/usr/bin/env python3
"""Recovers a material and an environment together from one image, on dirt_amd (MI355X): the sphere of fit_environment_fused.py
with an albedo, a roughness and a metalness that vary over its surface, rendered through `rasterise_deferred` into a 12-channel
G-buffer (mask, normal, position, albedo, roughness, metalness) and lit by `shading.shade_gbuffer_ibl`, split-sum image-based
lighting in one kernel.  Every step the shader turns the learnable environment into its two filtered forms --
`texture.prefilter_cube` for the specular half, `texture.convolve_cube(kind='lambert')` on a small mip for the irradiance -- so
the gradient of the image reaches the environment through both, and the per-vertex albedo and material through the G-buffer.
The table of `lighting.environment_brdf` is built once.

    python examples/fit_material_environment_fused.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import dirt_amd as dirt  # noqa: E402
from dirt_amd import lighting, matrices, shading, texture  # noqa: E402
from fit_environment_fused import CAMERA, SIZE, build_sphere, true_environment  # noqa: E402

CHANNELS = 12
LAYOUT = dict(mask=0, normals=1, positions=4, colors=7, material=10)
BACKGROUND = (0.05, 0.05, 0.1)
IRRADIANCE_LEVEL = 2      # the mip of the environment the irradiance is convolved from: 16 -> 4 texels along an edge
TABLE = 32


def true_material(vertices):
    """-> (albedo [V, 3], material [V, 2]): red to green along x; polished at the bottom, rough at the top; metal on one side"""
    x, y, z = vertices.unbind(-1)
    albedo = torch.stack([0.5 + 0.4 * x, 0.5 - 0.4 * x, 0.4 + 0.2 * z], -1)
    return albedo, torch.stack([0.45 + 0.35 * y, 0.5 + 0.45 * z], -1)


def filtered(environment):
    """the two forms of the environment the shader reads -> (the GGX-prefiltered pyramid, the irradiance cube)"""
    mip = texture.cube_pyramid(environment).level(IRRADIANCE_LEVEL)
    return texture.prefilter_cube(environment), texture.convolve_cube(mip, kind='lambert')


class Scene:
    def __init__(self, device):
        self.vertices, self.faces = (torch.from_numpy(a).to(device) for a in build_sphere())
        self.albedo, self.material = true_material(self.vertices)

    def clip(self, width, height):
        dev = self.vertices.device
        view = matrices.translation(torch.tensor([-x for x in CAMERA], device=dev))
        projection = matrices.perspective_projection(near=0.1, far=20., right=0.05, aspect=float(height) / width).to(dev)
        v4 = torch.cat([self.vertices, torch.ones_like(self.vertices[:, :1])], dim=1)
        return (v4 @ view) @ projection

    def attributes(self, albedo=None, material=None):
        v = self.vertices
        return torch.cat([torch.ones_like(v[:, :1]), lighting.vertex_normals(v, self.faces), v, self.albedo if albedo is None else albedo,
                          self.material if material is None else material], dim=1)


def render(scene, environment, albedo, material, brdf, width, height):
    def shader_fn(gbuffer, env):
        pyramid, irradiance = filtered(env)
        # the background (mask 0) has a zero normal: no irradiance, and the pixel is the background colour
        return shading.shade_gbuffer_ibl(gbuffer, pyramid, irradiance, brdf, camera_position=CAMERA, background=BACKGROUND, **LAYOUT)

    return dirt.rasterise_deferred(background_attributes=torch.zeros([height, width, CHANNELS], device=environment.device),
                                   vertices=scene.clip(width, height), vertex_attributes=scene.attributes(albedo, material), faces=scene.faces,
                                   shader_fn=shader_fn, shader_additional_inputs=[environment])


def fit(width=160, height=120, steps=80, rate=0.05, device=None):
    """-> (losses per step, mean |environment - truth| over the texels, before and after)"""
    dev = device or torch.device('cuda', 0)
    scene = Scene(dev)
    brdf = lighting.environment_brdf(TABLE).to(dev)
    truth = true_environment(SIZE, dev)
    target = render(scene, truth, scene.albedo, scene.material, brdf, width, height).detach()
    environment = torch.full_like(truth, 0.5).requires_grad_(True)
    albedo = torch.full_like(scene.albedo, 0.5).requires_grad_(True)
    material = torch.full_like(scene.material, 0.5).requires_grad_(True)
    optimiser = torch.optim.Adam([environment, albedo, material], lr=rate)
    before = float((environment.detach() - truth).abs().mean())
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        loss = ((render(scene, environment, albedo, material, brdf, width, height) - target) ** 2).mean()
        loss.backward()
        optimiser.step()
        with torch.no_grad():
            albedo.clamp_(0., 1.), material.clamp_(0., 1.), environment.clamp_(min=0.)
        losses.append(float(loss.detach()))
    return losses, before, float((environment.detach() - truth).abs().mean())


def main():
    losses, before, after = fit()
    print('losses: ' + ' '.join('%.3e' % x for x in losses[::10] + losses[-1:]))
    print('loss %.3e -> %.3e in %d steps; mean |environment - truth| %.3f -> %.3f' % (losses[0], losses[-1], len(losses), before, after))
    assert losses[-1] < losses[0] and after < before, 'the fit did not bring the loss and the environment error down'


if __name__ == '__main__':
    main()
