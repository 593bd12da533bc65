"""The fused image-based G-buffer lighting (dirt_amd.shading.shade_gbuffer_ibl) against the route available before it, `composed`:
the reflection, the dots and the clamps in torch, texture.sample_cube_pyramid for the specular look-up, texture.sample_texture_cube
for the irradiance, the table look-up and the combine in torch.  Timed with HIP events after warm-up, in one process, the two
legs alternating (the method of tools/bench_shade.py), on a 1024 x 1024 x 12 G-buffer with a 6 x 256^2 x 3 environment (its
prefiltered pyramid made once, outside the timed region; the irradiance from its 16-texel mip; a 32^2 table):
      forward            the call alone through the public API, nothing requiring a gradient;
      forward_backward   forward + backward with gradients to the G-buffer, the three parameters, the pyramid and the irradiance;
      c_forward, c_backward   the fused route's two C entry points alone, on buffers made once (every gradient wanted), and the
                         backward with neither cube's gradient wanted, and with one of them: where its time goes.
The G-buffer's positions, normals and roughness are smooth fields, as a rendered surface's are.
Every figure is the median over `repeats` blocks of `steps` steps, with the spread (min .. max) of the blocks.  No ratio is
required of this tool: it records what it reads.
usage (GPU box): python tools/bench_shade_ibl.py [steps] [repeats]     (prints one JSON line, writes profiles/shade_ibl.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dirt_amd import _lib, lighting, shading, texture  # noqa: E402
from bench_shade import time_alternating  # noqa: E402

LAYOUT = dict(mask=0, positions=1, colors=4, normals=7, material=10)


def composed(gbuffer, specular, irradiance, brdf, *, colors, material, normals, positions, camera_position, mask=None,
             intensity=(1., 1., 1.), background=(0., 0., 0.), clamp=(0., 1.), min_roughness=0.04, dielectric_f0=0.04):
    """`shade_gbuffer_ibl` for channel offsets, composed of the ops the library had before it: what
    `lighting.image_based_lighting` specifies, with the two cube look-ups by the fused look-up kernels"""
    as_t = lambda x: x if isinstance(x, torch.Tensor) else torch.tensor(x, dtype=torch.float32, device=gbuffer.device)   # noqa: E731
    unit = lambda x: torch.nn.functional.normalize(x, dim=-1, eps=1.e-12)   # noqa: E731
    c, n, p = gbuffer[..., colors:colors + 3], gbuffer[..., normals:normals + 3], gbuffer[..., positions:positions + 3]
    r, mu = gbuffer[..., material], gbuffer[..., material + 1:material + 2]
    m = gbuffer[..., mask:mask + 1] if mask is not None else torch.ones_like(gbuffer[..., :1])
    N, v = unit(n), unit(as_t(camera_position) - p)
    nv_raw = (N * v).sum(-1)
    nv = nv_raw.clamp(min=0.)
    rho = r.clamp(min_roughness, 1.)
    f0 = dielectric_f0 * (1. - mu) + c * mu
    reflected = (2. * nv_raw)[..., None] * N - v
    size = int(brdf.shape[0])
    ab = lighting._table_lookup(brdf, (rho * float(size) - 0.5).clamp(0., float(size - 1)), (nv * float(size) - 0.5).clamp(0., float(size - 1)))
    s = f0 * ab[..., :1] + ab[..., 1:]
    spec = texture.sample_cube_pyramid(specular, reflected, rho * float(specular.levels - 1))
    e = texture.sample_texture_cube(irradiance, n)
    lit = as_t(intensity) * (((1. - s) * (1. - mu)) * c * e + s * spec)
    pre = lit * m + as_t(background) * (1. - m)
    return torch.clamp(pre, clamp[0], clamp[1]) if clamp is not None else pre


def main():
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    steps = int(args[0]) if args else 10
    repeats = int(args[1]) if len(args) > 1 else 7
    t = lambda x: torch.tensor(x, dtype=torch.float32, device=dev, requires_grad=True)   # noqa: E731
    intensity, camera, background = t([0.9, 0.8, 1.0]), t([0.3, -0.2, 4.]), t([0., 0., 0.3])
    h = w = 1024
    c = 12
    environment = torch.rand(6, 256, 256, 3, device=dev)
    with torch.no_grad():
        packed = texture.prefilter_cube(environment).packed.clone()
        irr = texture.convolve_cube(texture.cube_pyramid(environment).level(4).contiguous(), kind='lambert').contiguous()
    levels = 9
    packed.requires_grad_(True), irr.requires_grad_(True)
    pyramid = texture.CubePyramid(packed, 256, 3, levels, tuple(k / (levels - 1) for k in range(levels)))
    brdf = lighting.environment_brdf(32).to(dev)
    g = torch.rand(h, w, c, device=dev)
    g[..., 0] = (g[..., 0] < 0.7).float()
    # smooth fields of positions, normals and roughness, as a rendered surface has: neighbouring pixels look up neighbouring
    # texels, which is what the scatter's LDS patch is made for (albedo, metalness and the mask stay noise)
    yy, xx = torch.meshgrid(torch.linspace(-1., 1., h, device=dev), torch.linspace(-1., 1., w, device=dev), indexing='ij')
    g[..., 1:4] = torch.stack([xx, yy, 0.2 * torch.sin(2. * xx) * torch.cos(2. * yy)], -1)
    g[..., 10] = 0.5 + 0.3 * torch.sin(4. * xx + yy)
    g[..., 7:10] = torch.nn.functional.normalize(torch.stack([torch.sin(3. * xx), torch.sin(2. * yy), 0.6 + 0.3 * torch.cos(xx + yy)], -1), dim=-1)
    d = torch.from_numpy(rng.standard_normal((h, w, 3)).astype(np.float32)).to(dev)
    params = [intensity, camera, background, packed, irr]
    kw = dict(intensity=intensity, camera_position=camera, background=background, **LAYOUT)
    out = {'steps': steps, 'repeats': repeats, 'gbuffer': [h, w, c], 'environment': [6, 256, 256, 3], 'levels': levels, 'irradiance': int(irr.shape[1]),
           'table': 32}
    for name, leaf in (('forward', g.detach()), ('forward_backward', g.detach().requires_grad_(True))):
        def leg(fn, leaf=leaf, name=name):
            def step():
                if name == 'forward':
                    with torch.no_grad():
                        fn(leaf, pyramid, irr, brdf, **kw)
                    return
                leaf.grad = None
                for x in params:
                    x.grad = None
                fn(leaf, pyramid, irr, brdf, **kw).backward(d)
            return step

        r = time_alternating({'composed': leg(composed), 'fused': leg(shading.shade_gbuffer_ibl)}, steps, repeats)
        r['speedup'] = r['composed']['ms'] / r['fused']['ms']
        out[name] = r
    # the two C entry points alone
    lib = _lib.load()
    block = torch.cat([intensity, background, camera]).detach()[None].contiguous()
    bufs = dict(out=torch.empty(h, w, 3, device=dev), gg=torch.empty_like(g), gp=torch.empty(1, 9, device=dev), gs=torch.empty_like(packed),
                gi=torch.empty_like(irr))
    nbytes = lib.dirt_shade_ibl_scratch_bytes(1, h, w)
    scratch = torch.empty(nbytes // 4, device=dev)
    tail = (1, h, w, c, 0, 0, LAYOUT['colors'], LAYOUT['material'], LAYOUT['normals'], LAYOUT['positions'], LAYOUT['mask'], 1, 256, levels, int(irr.shape[1]),
            32, 0.04, 0.04, 0., 1., _lib.SHADE_CLAMP, None)
    pk, ir = packed.detach(), irr.detach()

    def c_forward():
        _lib.check(lib.dirt_shade_ibl_forward(g.data_ptr(), None, None, block.data_ptr(), pk.data_ptr(), ir.data_ptr(), brdf.data_ptr(),
                                              bufs['out'].data_ptr(), *tail))

    def c_backward():
        _lib.check(lib.dirt_shade_ibl_backward(g.data_ptr(), None, None, block.data_ptr(), pk.data_ptr(), ir.data_ptr(), brdf.data_ptr(), d.data_ptr(),
                                               bufs['gg'].data_ptr(), None, None, bufs['gp'].data_ptr(), bufs['gs'].data_ptr(), bufs['gi'].data_ptr(),
                                               scratch.data_ptr(), nbytes, *tail))

    def c_backward_part(pyramid_too, irradiance_too):
        def call():
            _lib.check(lib.dirt_shade_ibl_backward(g.data_ptr(), None, None, block.data_ptr(), pk.data_ptr(), ir.data_ptr(), brdf.data_ptr(),
                                                   d.data_ptr(), bufs['gg'].data_ptr(), None, None, bufs['gp'].data_ptr(),
                                                   bufs['gs'].data_ptr() if pyramid_too else None, bufs['gi'].data_ptr() if irradiance_too else None,
                                                   scratch.data_ptr(), nbytes, *tail))
        return call

    out['c_calls'] = time_alternating({'c_forward': c_forward, 'c_backward': c_backward, 'c_backward_without_the_cubes': c_backward_part(False, False),
                                       'c_backward_pyramid_only': c_backward_part(True, False),
                                       'c_backward_irradiance_only': c_backward_part(False, True)}, steps, repeats)
    print(json.dumps(out))
    with open(os.path.join(ROOT, 'profiles', 'shade_ibl.json'), 'w') as fh:
        json.dump({'note': 'MI355X; HIP events, legs alternating in one process, median [min, max] of %d blocks of %d steps '
                           '(tools/bench_shade_ibl.py)' % (repeats, steps), 'bench_shade_ibl': out}, fh, indent=1)


if __name__ == '__main__':
    main()
