"""GPU box: the cube-map look-up (dirt_texture_cube.hip) -- HIP-event times of `texture.sample_texture_cube` and of its backward
at 2048^2 look-ups from a 6 x 512^2 x 3 cube, bilinear and trilinear, and beside them, measured in the same process at the same
pixel count: `sample_texture_uv` from a 512^2 x 3 texture (the flat look-up the kernels are modelled on), the pure-torch form
(`directions_to_cube_indices` + `sample_cube`) and the lat-long work-around (atan2 / acos in torch, then
`sample_texture_uv(mode='repeat')` from a 1024 x 2048 x 3 panorama, which holds the cube's texel count).
The directions are what a G-buffer holds: the reflection of the view vector on a sphere that fills the frame, read in place from
channels 4:7 of a 10-channel buffer; the corners of the frame are background, direction (0, 0, 0).  Every figure is the mean of
`n` calls between two events after 5 warm-up calls, through the public API (so a backward is one torch.autograd.grad over a
retained graph: the kernels plus the autograd node's allocations); the C ABI calls alone are timed too, for the cube look-up.
usage: python tools/bench_texture_cube.py [json path, default profiles/texture_cube.json] [--pixels 2048] [--size 512]"""
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dirt_amd import _lib, rasterise_ops as _ops, texture  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
out_path = next((a for a in argv if a.endswith('.json')), os.path.join(ROOT, 'profiles', 'texture_cube.json'))
P = int(argv[argv.index('--pixels') + 1]) if '--pixels' in argv else 2048
N = int(argv[argv.index('--size') + 1]) if '--size' in argv else 512
CT = 3
if not torch.cuda.is_available():
    sys.exit('bench_texture_cube.py measures on an MI355X; no GPU found')
dev = torch.device('cuda:0')
lib = _lib.load()
stream = _ops._stream_handle(dev)


def timed(fn, n=30):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3   # us


def forward_backward(make_out, leaves, g):
    """-> (forward us, backward us) of out = make_out() and torch.autograd.grad(out, leaves, g)"""
    out = make_out()
    t_fwd = timed(make_out)
    t_bwd = timed(lambda: torch.autograd.grad(out, leaves, g, retain_graph=True))
    return t_fwd, t_bwd


rng = np.random.default_rng(0)
ys, xs = np.meshgrid(np.linspace(-1.05, 1.05, P, dtype=np.float32), np.linspace(-1.05, 1.05, P, dtype=np.float32), indexing='ij')
inside = xs * xs + ys * ys < 1
nz = np.sqrt(np.where(inside, 1 - xs * xs - ys * ys, 0)).astype(np.float32)
normal = np.stack([xs, -ys, nz], -1) * inside[..., None]
view = np.array([0, 0, -1], np.float32)
reflected = (view - 2 * (normal @ view)[..., None] * normal) * inside[..., None]
gbuf = np.zeros((P, P, 10), np.float32)
gbuf[..., 0] = inside
gbuf[..., 4:7] = reflected
gbuf[..., 1] = (xs * 0.5 + 0.5) * (P / N / 4)   # the flat look-up's (u, v): a smooth field at ~1 texel per pixel, in place from channels 1:3
gbuf[..., 2] = (ys * 0.5 + 0.5) * (P / N / 4)
gb = torch.from_numpy(gbuf).to(dev).requires_grad_(True)
dirs = gb[..., 4:7]
cube = torch.from_numpy(rng.uniform(0, 1, (6, N, N, CT)).astype(np.float32)).to(dev).requires_grad_(True)
flat = torch.from_numpy(rng.uniform(0, 1, (N, N, CT)).astype(np.float32)).to(dev).requires_grad_(True)
pano = torch.from_numpy(rng.uniform(0, 1, (2 * N, 4 * N, CT)).astype(np.float32)).to(dev).requires_grad_(True)
g = torch.from_numpy(rng.standard_normal((P, P, CT)).astype(np.float32)).to(dev)
levels = lib.dirt_texture_mip_levels(N, N, CT, -1, None)
lod = torch.from_numpy((xs * 0.5 + 0.5) * (levels - 1) * 0.5).to(dev).requires_grad_(True)   # a roughness ramp across the frame: levels 0 .. (L - 1) / 2
uvs = gb[..., 1:3]


def latlong(d):
    """direction -> (u, v) of an equirectangular panorama, in torch (the work-around the cube look-up replaces)"""
    n = torch.nn.functional.normalize(d, dim=-1)
    u = torch.atan2(n[..., 0], -n[..., 2]) / (2 * math.pi) + 0.5
    v = torch.acos(n[..., 1].clamp(-1 + 1e-6, 1 - 1e-6)) / math.pi
    return torch.stack([u, v], -1)


results = {}
results['cube_bilinear'] = forward_backward(lambda: texture.sample_texture_cube(cube, dirs), [cube, gb], g)
results['cube_trilinear'] = forward_backward(lambda: texture.sample_texture_cube(cube, dirs, 'trilinear', lod=lod), [cube, gb, lod], g)
results['uv_bilinear'] = forward_backward(lambda: texture.sample_texture_uv(flat, uvs), [flat, gb], g)
results['torch_form'] = forward_backward(lambda: texture.sample_cube(cube, *texture.directions_to_cube_indices(dirs, N)), [cube, gb], g)
results['latlong_workaround'] = forward_backward(lambda: texture.sample_texture_uv(pano, latlong(dirs), 'repeat'), [pano, gb], g)

# the C ABI calls alone: no allocation, no autograd node
with torch.no_grad():
    floats = ctypes.c_longlong(0)
    lib.dirt_texture_mip_levels(N, N, CT, -1, ctypes.byref(floats))
    pyr, scratch = torch.empty(6, floats.value, device=dev), torch.empty(6, floats.value, device=dev)
    out, gd, gl, gc = torch.empty(P, P, CT, device=dev), torch.empty(P, P, 3, device=dev), torch.empty(P, P, device=dev), torch.empty_like(cube)
    c0, d0, l0 = cube.detach(), dirs.detach(), lod.detach()
    assert lib.dirt_texture_mip_build_batch(c0.data_ptr(), pyr.data_ptr(), 6, N, N, CT, levels, stream) == 0
    calls = {
        'cube_bilinear_forward': lambda: lib.dirt_texture_cube_forward(c0.data_ptr(), d0.data_ptr(), None, out.data_ptr(), P * P, N, CT, 1, 10, 0.0, 0, stream),
        'cube_bilinear_backward': lambda: lib.dirt_texture_cube_backward(c0.data_ptr(), d0.data_ptr(), None, g.data_ptr(), gc.data_ptr(), gd.data_ptr(), None, P, P, N, CT, 1, 10, 3, 0.0, 0, stream),
        'cube_pyramid_build': lambda: lib.dirt_texture_mip_build_batch(c0.data_ptr(), pyr.data_ptr(), 6, N, N, CT, levels, stream),
        'cube_trilinear_forward': lambda: lib.dirt_texture_cube_forward(pyr.data_ptr(), d0.data_ptr(), l0.data_ptr(), out.data_ptr(), P * P, N, CT, levels, 10, 0.0, 0, stream),
        'cube_trilinear_backward': lambda: lib.dirt_texture_cube_backward(pyr.data_ptr(), d0.data_ptr(), l0.data_ptr(), g.data_ptr(), scratch.data_ptr(), gd.data_ptr(), gl.data_ptr(), P, P, N, CT, levels, 10, 3, 0.0, 0, stream),
        'cube_pyramid_collapse': lambda: lib.dirt_texture_mip_collapse_batch(scratch.data_ptr(), gc.data_ptr(), 6, N, N, CT, levels, stream),
    }
    for name, call in calls.items():
        assert call() == 0, (name, lib.dirt_texture_last_error())
    c_abi = {name + '_us': timed(call) for name, call in calls.items()}

report = {'workload': '%d x %d look-ups (%.0f %% on the sphere) from a 6 x %d x %d x %d cube, directions in place from a 10-channel G-buffer' % (P, P, 100 * inside.mean(), N, N, CT),
          'levels': levels, 'calls_per_figure': 30,
          'public_api_us': {k: {'forward': v[0], 'backward': v[1]} for k, v in results.items()},
          'c_abi_us': c_abi,
          'ratios': {'cube_bilinear_over_uv_bilinear': {'forward': results['cube_bilinear'][0] / results['uv_bilinear'][0], 'backward': results['cube_bilinear'][1] / results['uv_bilinear'][1]},
                     'torch_form_over_cube_bilinear': {'forward': results['torch_form'][0] / results['cube_bilinear'][0], 'backward': results['torch_form'][1] / results['cube_bilinear'][1]},
                     'latlong_workaround_over_cube_bilinear': {'forward': results['latlong_workaround'][0] / results['cube_bilinear'][0], 'backward': results['latlong_workaround'][1] / results['cube_bilinear'][1]},
                     'cube_trilinear_over_cube_bilinear': {'forward': results['cube_trilinear'][0] / results['cube_bilinear'][0], 'backward': results['cube_trilinear'][1] / results['cube_bilinear'][1]},
                     'c_abi_trilinear_backward_over_bilinear_backward': c_abi['cube_trilinear_backward_us'] / c_abi['cube_bilinear_backward_us']}}
print(json.dumps(report))
json.dump(report, open(out_path, 'w'), indent=1)
