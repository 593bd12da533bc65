"""GPU box: the environment prefilter (dirt_envmap.hip) -- HIP-event times of dirt_envmap_filter_forward and _backward per level of the
pyramids of a 6 x 256^2 x 3 and a 6 x 512^2 x 3 cube at the default roughness k / (L - 1) (level 0, roughness 0, is a copy and is
not timed), of `texture.prefilter_cube` and its backward as a whole, and of `convolve_cube` beside `convolve_cube_dense` (the dense
[6 n^2, 6 n^2] matrix in torch on the GPU) at the sizes where that matrix fits, n <= 64.  Per level it also reports the share of
tile pairs the kernel's cone test drops -- the test restated here in numpy float64 -- and the texel pairs of the remaining tile
pairs per second.  Every figure is the mean of `n` calls between two events after 2 warm-up calls.  No threshold: a first measurement.
usage: python tools/bench_envmap.py [json path, default profiles/envmap.json] [--sizes 256,512]"""
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
out_path = next((a for a in argv if a.endswith('.json')), os.path.join(ROOT, 'profiles', 'envmap.json'))
SIZES = [int(s) for s in argv[argv.index('--sizes') + 1].split(',')] if '--sizes' in argv else [256, 512]
CT, TILE, MARGIN = 3, 16, 1e-4
if not torch.cuda.is_available():
    sys.exit('bench_envmap.py measures on an MI355X; no GPU found')
dev = torch.device('cuda:0')
lib = _lib.load()
stream = _ops._stream_handle(dev)


def timed(fn, n=5):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3   # us


def texel_direction(face, r, c, n):
    sc, tc = 2. * (c + 0.5) / n - 1., 2. * (r + 0.5) / n - 1.
    one = np.ones_like(sc)
    v = [(one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one)]
    v = np.stack([np.choose(face, [x[i] for x in v]) for i in range(3)], -1)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def angle(a, b):
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1))


def cone_test(n, roughness):
    """The kernel's tile cull in float64 -> (live tile pairs, all tile pairs, texel pairs of the live tile pairs)."""
    a2 = roughness ** 4
    cut = math.acos(math.sqrt((1. - 16. * a2) / (1. - a2))) if 16. * a2 < 1. else math.pi / 2
    tiles = -(-n // TILE)
    f, ty, tx = (x.reshape(-1) for x in np.meshgrid(np.arange(6), np.arange(tiles), np.arange(tiles), indexing='ij'))
    r0, c0 = (ty * TILE).astype(np.float64), (tx * TILE).astype(np.float64)
    r1, c1 = np.minimum(ty * TILE + TILE, n) - 1., np.minimum(tx * TILE + TILE, n) - 1.
    axis = texel_direction(f, 0.5 * (r0 + r1), 0.5 * (c0 + c1), n)
    half = np.max([angle(axis, texel_direction(f, r, c, n)) for r in (r0, r1) for c in (c0, c1)], 0)
    live = angle(axis[:, None], axis[None, :]) - half[:, None] - half[None, :] - MARGIN < cut
    texels = (r1 - r0 + 1) * (c1 - c0 + 1)
    return int(live.sum()), live.size, float((live * texels[:, None] * texels[None, :]).sum())


rng = np.random.default_rng(0)
report = {'channels': CT, 'calls_per_figure': 5, 'cubes': {}, 'dense': {}}
with torch.no_grad():
    for N in SIZES:
        cube = torch.from_numpy(rng.uniform(0, 1, (6, N, N, CT)).astype(np.float32)).to(dev)
        box = texture.cube_pyramid(cube)
        floats = box.packed.shape[1]
        dst, gsrc = torch.empty_like(box.packed), torch.empty_like(box.packed)
        g = torch.randn_like(box.packed)
        levels = []
        for k in range(1, box.levels):
            r, nk = k / (box.levels - 1), N >> k
            o = (N * N - nk * nk) // 3 * 4 * CT
            norm = torch.empty(6, nk, nk, device=dev)
            args = (nk, CT, floats, r * r, _lib.ENVMAP_GGX, stream)
            fwd = lambda: lib.dirt_envmap_filter_forward(box.packed[0, o:].data_ptr(), dst[0, o:].data_ptr(), norm.data_ptr(), *args)   # noqa: E731
            bwd = lambda: lib.dirt_envmap_filter_backward(g[0, o:].data_ptr(), norm.data_ptr(), gsrc[0, o:].data_ptr(), *args)           # noqa: E731
            assert fwd() == 0 and bwd() == 0, lib.dirt_texture_last_error()
            t_f, t_b = timed(fwd), timed(bwd)
            live, pairs, texel_pairs = cone_test(nk, r)
            levels.append({'level': k, 'size': nk, 'roughness': r, 'forward_us': t_f, 'backward_us': t_b, 'tile_pairs': pairs, 'tile_pairs_culled_share': 1. - live / pairs,
                           'live_texel_pairs': texel_pairs, 'live_texel_pairs_per_s_forward': texel_pairs / (t_f * 1e-6), 'live_texel_pairs_per_s_backward': texel_pairs / (t_b * 1e-6)})
        entry = {'levels': levels, 'filters_forward_us': sum(x['forward_us'] for x in levels), 'filters_backward_us': sum(x['backward_us'] for x in levels)}
        with torch.enable_grad():
            leaf = cube.clone().requires_grad_(True)
            pyr = texture.prefilter_cube(leaf)
            entry['prefilter_cube_forward_us'] = timed(lambda: texture.prefilter_cube(leaf))
            entry['prefilter_cube_backward_us'] = timed(lambda: torch.autograd.grad(pyr.packed, leaf, g, retain_graph=True))
        report['cubes']['6x%dx%dx%d' % (N, N, CT)] = entry

for n in (16, 32, 64):
    cube = torch.from_numpy(rng.uniform(0, 1, (6, n, n, CT)).astype(np.float32)).to(dev).requires_grad_(True)
    g = torch.randn(6, n, n, CT, device=dev)
    row = {}
    for name, f in (('convolve_cube', texture.convolve_cube), ('convolve_cube_dense', texture.convolve_cube_dense)):
        out = f(cube, 0.5)
        row[name] = {'forward_us': timed(lambda: f(cube, 0.5)), 'backward_us': timed(lambda: torch.autograd.grad(out, cube, g, retain_graph=True))}
    row['dense_over_kernel_forward'] = row['convolve_cube_dense']['forward_us'] / row['convolve_cube']['forward_us']
    report['dense']['n=%d roughness 0.5' % n] = row

print(json.dumps(report))
json.dump(report, open(out_path, 'w'), indent=1)
